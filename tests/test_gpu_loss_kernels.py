"""The loss kernels of csrc/pointwise.hip at kernel level, at sizes where their slab splits, caps and wraps.

The entry points are called directly and in the order the autograd functions of selective_loss.py call them —
partials, selunet_reduce_rows, finalize, bwd — so the slab, the fp64 sums and `state` are visible. The other
kernel-level cases (tests/golden/loss_cases*.npz, test_ce_loss_kernels_against_torch) have P <= 1024: one
workgroup, one slab row, chunk = P. Here P runs over {1, 255, 4096, 4097, 3*4096 + 77, 1024*4096 + 4099}: the chunk
split across rows, the ragged last chunk, the 1024-row cap with a chunk that is no multiple of 256, and the
backward's capped grid (8192 workgroups) wrapping. CE: image boundaries inside chunks, C = 8 (the unroll bound).

Bounds: tests/test_gpu_loss_cases.py's TOL = 1e-5 for the BCE forms (scalars relative to max(1, |value|),
gradients to the tensor's maximum), test_ce_loss_kernels_against_torch's for the CE forms (loss 1e-5, coverage
1e-6, gradients 1e-4), against the oracle's forms evaluated in fp64. The counting tests have no tolerance.
Every figure is printed as a line "coverage: ..." (collected in profiles/pointwise_coverage.txt).
"""
import numpy as np
import pytest
import torch

from oracle import unet_b_cpu as O
from selectivenet_for_semantic_segmentation_binary_amd import _lib as K
from tests import _golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5                                   # tests/test_gpu_loss_cases.py
CE_LOSS, CE_COV, CE_GRAD = 1e-5, 1e-6, 1e-4  # tests/test_gpu_ce.py::test_ce_loss_kernels_against_torch
TC = 0.8                                     # target coverage (the reference's default)

# The launch constants csrc/pointwise.hip does not export (line numbers of that file)
TPB = 256        # :39   constexpr int TPB
BWD_CAP = 8192   # :2168 :2199 :2324 :2354 grid_for(p, 8192) of the four backward launchers
P_LIST = [1, 255, 4096, 4097, 3 * 4096 + 77, 1024 * 4096 + 4099]
CE_SHAPES = [(5, 8, 1639), (3, 3, 2731), (3, 2, 1399469)]
P_A, P_B = 3 * 4096 + 77, 4097               # the two data-parallel parts
SENTINEL = -7.25e11


def cdiv(a, b):
    return -(-a // b)


def note(what, err, bound):
    print(f"coverage: {what}: {float(err):.2e} (bound {bound:.1e})")


def scal(a, b):
    return abs(a - b) / max(1.0, abs(b))


def regime(p):
    """(slab rows, chunk) of a loss partials launch, from the exported query; asserts what the size is there for."""
    rows = K.query("selunet_loss_slab_rows", p)
    assert rows == max(1, min(cdiv(p, 4096), 1024))
    chunk = cdiv(p, rows)
    if p > 1024 * 4096:
        assert rows == 1024 and chunk % TPB != 0 and p > BWD_CAP * TPB  # capped rows; the backward grid wraps
    if p in (4097, 3 * 4096 + 77) or p > 1024 * 4096:
        assert rows > 1 and 0 < p - (rows - 1) * chunk < chunk         # several rows, a ragged last chunk
    return rows, chunk


def dev(a):
    return torch.as_tensor(a).to(DEV).contiguous()


class Guarded:
    """A device buffer of `numel` floats (NaN) between two bands of 64 sentinel floats."""

    def __init__(self, numel):
        self.n = numel
        self.buf = torch.full((numel + 128,), SENTINEL, device=DEV)
        self.buf[64:64 + numel] = float("nan")
        self.ptr = self.buf.data_ptr() + 64 * 4

    def get(self):
        """The written values; the bands must be untouched and every element written (the inputs are finite)."""
        b = self.buf.cpu()
        assert bool((b[:64] == SENTINEL).all()) and bool((b[-64:] == SENTINEL).all())
        v = b[64:64 + self.n].clone()
        assert not torch.isnan(v).any()
        return v


def reduce_rows(slab, cols):
    rows = slab.shape[0]
    sums = torch.full((cols,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(K.query("selunet_reduce_ws_bytes", cols) // 8, dtype=torch.float64, device=DEV)
    K.call("selunet_reduce_rows", K.ptr(slab), rows, cols, K.ptr(ws), K.ptr(sums), None, K.stream_ptr())
    return sums


def selective_finalize(sums, p_global, lamb):
    loss, cov = torch.full((), float("nan"), device=DEV), torch.full((), float("nan"), device=DEV)
    state = torch.full((4,), float("nan"), device=DEV)
    K.call("selunet_selective_finalize", K.ptr(sums), float(p_global), float(lamb), TC, K.ptr(loss), K.ptr(cov),
           K.ptr(state), K.stream_ptr())
    return loss, cov, state


def mean_finalize(sums, p_global):
    loss = torch.full((), float("nan"), device=DEV)
    K.call("selunet_bce_finalize", K.ptr(sums), float(p_global), K.ptr(loss), K.stream_ptr())
    return loss


class BForm:
    """The BCE forms on flat [P] tensors: selunet_selective_* / selunet_bce_*."""

    def __init__(self, out, sel, tgt):
        self.o, self.s, self.t = dev(out), dev(sel), dev(tgt)
        self.p = self.o.numel()
        self.rows, self.chunk = regime(self.p)

    def partials(self, hard=False):
        slab = torch.full((self.rows, 2), float("nan"), device=DEV)
        K.call("selunet_selective_partials_hard" if hard else "selunet_selective_partials", K.ptr(self.o),
               K.ptr(self.s), K.ptr(self.t), self.p, K.ptr(slab), K.stream_ptr())
        return slab

    def bwd(self, state, lamb, hard=False, gl=None, gc=None):
        d_out, d_sel = Guarded(self.p), Guarded(self.p)
        if hard:
            K.call("selunet_selective_bwd_hard", K.ptr(self.o), K.ptr(self.s), K.ptr(self.t), self.p, K.ptr(state),
                   K.ptr(gl), d_out.ptr, d_sel.ptr, K.stream_ptr())
        else:
            K.call("selunet_selective_bwd", K.ptr(self.o), K.ptr(self.s), K.ptr(self.t), self.p, K.ptr(state),
                   float(lamb), K.ptr(gl), K.ptr(gc), d_out.ptr, d_sel.ptr, K.stream_ptr())
        torch.cuda.synchronize()
        return d_out.get(), d_sel.get()

    def mean_partials(self):
        slab = torch.full((self.rows, 1), float("nan"), device=DEV)
        K.call("selunet_bce_partials", K.ptr(self.o), K.ptr(self.t), self.p, K.ptr(slab), K.stream_ptr())
        return slab

    def mean_bwd(self, p_global, gl=None):
        d = Guarded(self.p)
        K.call("selunet_bce_bwd", K.ptr(self.o), K.ptr(self.t), self.p, float(p_global), K.ptr(gl), d.ptr,
               K.stream_ptr())
        torch.cuda.synchronize()
        return d.get()


class CEForm:
    """The CE forms on NCHW logits [n][C][hw], selection [n][2][hw], int64 target [n][hw]: selunet_ce_*."""

    def __init__(self, out, sel, tgt):
        self.o, self.s, self.t = dev(out), dev(sel), dev(tgt)
        self.n, self.c, self.hw = self.o.shape
        self.p = self.n * self.hw
        self.rows, self.chunk = regime(self.p)

    def partials(self, hard=False):
        slab = torch.full((self.rows, 2), float("nan"), device=DEV)
        K.call("selunet_ce_selective_partials_hard" if hard else "selunet_ce_selective_partials", K.ptr(self.o),
               K.ptr(self.s), K.ptr(self.t), self.n, self.c, self.hw, K.ptr(slab), K.stream_ptr())
        return slab

    def bwd(self, state, lamb, hard=False, gl=None, gc=None):
        d_out, d_sel = Guarded(self.o.numel()), Guarded(self.s.numel())
        if hard:
            K.call("selunet_ce_selective_bwd_hard", K.ptr(self.o), K.ptr(self.s), K.ptr(self.t), self.n, self.c,
                   self.hw, K.ptr(state), K.ptr(gl), d_out.ptr, d_sel.ptr, K.stream_ptr())
        else:
            K.call("selunet_ce_selective_bwd", K.ptr(self.o), K.ptr(self.s), K.ptr(self.t), self.n, self.c, self.hw,
                   K.ptr(state), float(lamb), K.ptr(gl), K.ptr(gc), d_out.ptr, d_sel.ptr, K.stream_ptr())
        torch.cuda.synchronize()
        return d_out.get().reshape(self.o.shape), d_sel.get().reshape(self.s.shape)

    def mean_partials(self):
        slab = torch.full((self.rows, 1), float("nan"), device=DEV)
        K.call("selunet_ce_partials", K.ptr(self.o), K.ptr(self.t), self.n, self.c, self.hw, K.ptr(slab),
               K.stream_ptr())
        return slab

    def mean_bwd(self, p_global, gl=None):
        d = Guarded(self.o.numel())
        K.call("selunet_ce_bwd", K.ptr(self.o), K.ptr(self.t), self.n, self.c, self.hw, float(p_global), K.ptr(gl),
               d.ptr, K.stream_ptr())
        torch.cuda.synchronize()
        return d.get().reshape(self.o.shape)


# ------------------------------------------------------------------ exactly-once counting
def needles(p, rows):
    """Pixel 0 and P - 1, both sides of every multiple of 4096, both sides of the chunk boundaries of the first, a
    middle and the last slab row, and 64 seeded positions."""
    chunk = cdiv(p, rows)
    pos = {0, p - 1}
    for b in range(4096, p, 4096):
        pos |= {b - 1, b}
    for r in {1, rows // 2, rows // 2 + 1, rows - 1}:
        b = r * chunk
        if 0 < b < p:
            pos |= {b - 1, b}
    pos |= set(np.random.default_rng(p).integers(0, p, 64).tolist())
    return np.array(sorted(pos), dtype=np.int64)


def check_counts(form, nd, lamb=8.0):
    """All-selected inputs with K needles of loss exactly 32: every partial is a small integer, exact in fp32."""
    p, k = form.p, len(nd)
    per_row = np.minimum(form.chunk, p - np.arange(form.rows) * form.chunk)  # pixels of each slab row
    hits = np.bincount(nd // form.chunk, minlength=form.rows)               # needles of each slab row
    want = np.float32(np.float64(32 * k) / np.float64(p))
    for hard in (False, True):
        slab = form.partials(hard)
        sums = reduce_rows(slab, 2)
        loss, cov, state = selective_finalize(sums, p, lamb)
        torch.cuda.synchronize()
        s = slab.cpu().numpy()
        assert np.array_equal(s[:, 0], per_row.astype(np.float32)) and np.array_equal(s[:, 1], 32.0 * hits)
        assert sums.cpu().tolist() == [float(p), 32.0 * k]
        assert state.cpu().tolist()[0] == float(p) and state.cpu().tolist()[3] == float(p)
        assert cov.item() == 1.0
        assert np.float32(loss.item()) == want, (loss.item(), want)
    slab = form.mean_partials()
    sums = reduce_rows(slab, 1)
    loss = mean_finalize(sums, p)
    torch.cuda.synchronize()
    assert np.array_equal(slab.cpu().numpy()[:, 0], 32.0 * hits) and sums.item() == 32.0 * k
    assert np.float32(loss.item()) == want, (loss.item(), want)
    return hits


def check_mirror(form, nd, lamb=8.0):
    """Nothing selected but the needles: S0 == K exactly, the risk is exactly 32."""
    p, k = form.p, len(nd)
    hits = np.bincount(nd // form.chunk, minlength=form.rows)
    for hard in (False, True):
        slab = form.partials(hard)
        sums = reduce_rows(slab, 2)
        loss, cov, state = selective_finalize(sums, p, lamb)
        torch.cuda.synchronize()
        s = slab.cpu().numpy()
        assert np.array_equal(s[:, 0], hits.astype(np.float32)) and np.array_equal(s[:, 1], 32.0 * hits)
        assert sums.cpu().tolist() == [float(k), 32.0 * k]
        st = state.cpu().tolist()
        assert st[0] == float(k) and st[1] == 32.0 and st[3] == float(p)
        assert np.float32(cov.item()) == np.float32(np.float64(k) / np.float64(p))
        d = max(float(np.float32(TC)) - k / p, 0.0)
        assert scal(loss.item(), 32.0 + lamb * d * d) <= TOL


@pytest.mark.parametrize("p", P_LIST)
def test_selective_and_bce_count_every_pixel_once(p):
    rows, _ = regime(p)
    nd = needles(p, rows)
    out = np.full(p, 200.0, np.float32)
    out[nd] = -32.0
    tgt = np.ones(p, np.float32)
    check_counts(BForm(out, np.full(p, 200.0, np.float32), tgt), nd)
    sel = np.full(p, -200.0, np.float32)
    sel[nd] = 200.0
    check_mirror(BForm(out, sel, tgt), nd)


@pytest.mark.parametrize("n,c,hw", CE_SHAPES)
def test_ce_counts_every_pixel_once(n, c, hw):
    """Target class 200, the others 0: se = 1 and the loss 0. A needle: target class -32, one other class 0, the
    rest -200: se = 1 (the terms below 2^-24 vanish), loss = 0 - (-32)."""
    p = n * hw
    rows, chunk = regime(p)
    # every image boundary falls inside a chunk; at 3 x 2731 the chunk is cdiv(8193, 3) = hw: there the image
    # boundaries are the chunk boundaries
    assert all(b % chunk for b in range(hw, p, hw)) if hw != 2731 else chunk == hw
    nd = needles(p, rows)
    rng = np.random.default_rng(c)
    tgt = rng.integers(0, c, p)
    out = np.zeros((n, c, hw), np.float32)
    flat = out.transpose(0, 2, 1).reshape(p, c)  # (a copy: [pixel][class])
    flat[np.arange(p), tgt] = 200.0
    flat[nd] = -200.0
    flat[nd, tgt[nd]] = -32.0
    flat[nd, (tgt[nd] + 1) % c] = 0.0
    out = np.ascontiguousarray(flat.reshape(n, hw, c).transpose(0, 2, 1))
    sel = np.zeros((n, 2, hw), np.float32)
    sel[:, 1] = 200.0
    check_counts(CEForm(out, sel, tgt.reshape(n, hw)), nd)
    sel1 = np.full(p, -200.0, np.float32)
    sel1[nd] = 200.0
    sel[:, 1] = sel1.reshape(n, hw)
    check_mirror(CEForm(out, sel, tgt.reshape(n, hw)), nd)


# ------------------------------------------------------------------ random inputs against the fp64 oracle
def away(a):
    """Selection logits kept at |g| >= 1e-3 (tests/golden/make_golden.py::hard_cases): no pixel on the hard cut."""
    return np.where(np.abs(a) < 1e-3, np.float32(1e-3) * np.sign(a + 1e-9), a).astype(np.float32)


def b_inputs(p, scale, sel_mean=0.5, seed=0):
    rng = np.random.default_rng([p, int(scale), seed])
    o = rng.normal(0, scale, p).astype(np.float32)
    s = away(rng.normal(sel_mean, scale, p).astype(np.float32))
    t = (rng.random(p) > 0.5).astype(np.float32)
    if p >= 255:  # saturated logits of both signs, on both targets, selected and not
        at = rng.choice(p, 16, replace=False)
        o[at] = np.tile(np.float32([90, -90, 104, -104]), 4)
        s[at] = np.repeat(np.float32([90, -90, 104, -104]), 4)
    return o, s, t


def b_ref(o, s, t, lamb, hard=False, gl=1.0, gc=0.0):
    """fp64: loss, coverage, the gradients of gl * loss + gc * coverage, and the plain BCE mean with its gradient."""
    o64, s64 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (o, s))
    t64 = torch.tensor(t, dtype=torch.float64)
    loss, cov = O.selective_risk_b_stable(o64, s64, t64, target_coverage=TC, lamb=lamb, hard_selection=hard)
    go, gs = torch.autograd.grad(gl * loss + gc * cov, (o64, s64), allow_unused=True)
    a64 = torch.tensor(o, dtype=torch.float64, requires_grad=True)
    bce = O.bce_with_logits_mean(a64, t64)
    (ga,) = torch.autograd.grad(bce, a64)
    return loss.item(), cov.item(), go.numpy(), (None if gs is None else gs.numpy()), bce.item(), ga.numpy()


def ce_inputs(n, c, hw, sel_mean=0.0, seed=7):
    g = torch.Generator().manual_seed(seed + c)
    out = (torch.randn(n, c, hw, generator=g) * 3).numpy()
    sel = (torch.randn(n, 2, hw, generator=g) * 2).numpy()
    sel[:, 1] = sel[:, 0] + away(sel[:, 1] - sel[:, 0] + np.float32(sel_mean))
    aux = (torch.randn(n, c, hw, generator=g) * 3).numpy()
    lab = torch.randint(0, c, (n, hw), generator=g).numpy()
    return out, sel, aux, lab


def ce_ref(out, sel, aux, lab, lamb, hard=False, gl=1.0, gc=0.0):
    n, c, hw = out.shape
    o64, s64, a64 = (torch.tensor(a, dtype=torch.float64).unsqueeze(-1).requires_grad_() for a in (out, sel, aux))
    t = torch.tensor(lab).unsqueeze(-1)
    loss, cov = O.selective_risk_ce_literal(o64, s64, t, target_coverage=TC, lamb=lamb, hard_selection=hard)
    go, gs = torch.autograd.grad(gl * loss + gc * cov, (o64, s64), allow_unused=True)
    ce = O.ce_mean(a64, t)
    (ga,) = torch.autograd.grad(ce, a64)
    sq = lambda g_: None if g_ is None else g_.squeeze(-1).numpy()  # noqa: E731
    return loss.item(), cov.item(), sq(go), sq(gs), ce.item(), sq(ga)


def run_selective(form, lamb, hard, p_global=None, gl=None, gc=None):
    slab = form.partials(hard)
    sums = reduce_rows(slab, 2)
    loss, cov, state = selective_finalize(sums, p_global or form.p, lamb)
    go, gs = form.bwd(state, lamb, hard, gl, gc)
    return dict(slab=slab.cpu(), sums=sums.cpu(), loss=loss.item(), cov=cov.item(), state=state.cpu(), go=go, gs=gs)


def run_mean(form, p_global=None, gl=None):
    slab = form.mean_partials()
    sums = reduce_rows(slab, 1)
    loss = mean_finalize(sums, p_global or form.p)
    return dict(slab=slab.cpu(), sums=sums.cpu(), loss=loss.item(), g=form.mean_bwd(p_global or form.p, gl))


def same_bits(a, b):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def check_b(tag, r, m, ref, hard):
    l64, c64, go64, gs64, bce64, ga64 = ref
    figs = dict(loss=scal(r["loss"], l64), cov=scal(r["cov"], c64), d_out=G.max_rel(r["go"].numpy(), go64),
                bce=scal(m["loss"], bce64), d_bce=G.max_rel(m["g"].numpy(), ga64))
    if hard:
        assert gs64 is None and float(r["gs"].abs().max()) == 0.0  # d_sel: all zeros
    else:
        figs["d_sel"] = G.max_rel(r["gs"].numpy(), gs64)
    for k, v in figs.items():
        note(f"{tag} {k}", v, TOL)
    assert np.isfinite(r["loss"]) and np.isfinite(m["loss"])
    assert all(v <= TOL for v in figs.values()), figs


def check_ce(tag, r, m, ref, hard):
    l64, c64, go64, gs64, ce64, ga64 = ref
    figs = [("loss", scal(r["loss"], l64), CE_LOSS), ("cov", abs(r["cov"] - c64), CE_COV),
            ("d_out", G.max_rel(r["go"].numpy(), go64), CE_GRAD), ("ce", scal(m["loss"], ce64), CE_LOSS),
            ("d_ce", G.max_rel(m["g"].numpy(), ga64), CE_GRAD)]
    if hard:
        assert gs64 is None and float(r["gs"].abs().max()) == 0.0
    else:
        figs.append(("d_sel", G.max_rel(r["gs"].numpy(), gs64), CE_GRAD))
    for k, v, b in figs:
        note(f"{tag} {k}", v, b)
    assert all(v < b for _, v, b in figs), figs


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("scale", [3, 20])
@pytest.mark.parametrize("p", P_LIST)
def test_selective_and_bce_against_fp64(p, scale, hard):
    """Logits ~ scale * N(0, 1) with +-90 and +-104 planted: finite, and loss, coverage and every element of both
    gradients within TOL of the stable form in fp64; two runs give the same bits (slab, sums, gradients); the
    gradients' guard bands stay untouched."""
    o, s, t = b_inputs(p, scale)
    form = BForm(o, s, t)
    r, m = run_selective(form, 8.0, hard), run_mean(form)
    same_bits(r, run_selective(form, 8.0, hard))
    same_bits(m, run_mean(form))
    check_b(f"selective/bce P={p} x{scale}{' hard' if hard else ''}", r, m, b_ref(o, s, t, 8.0, hard), hard)


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("n,c,hw", CE_SHAPES)
def test_ce_against_fp64(n, c, hw, hard):
    out, sel, aux, lab = ce_inputs(n, c, hw)
    form, mform = CEForm(out, sel, lab), CEForm(aux, sel, lab)
    r, m = run_selective(form, 8.0, hard), run_mean(mform)
    same_bits(r, run_selective(form, 8.0, hard))
    same_bits(m, run_mean(mform))
    check_ce(f"ce {n}x{c}x{hw}{' hard' if hard else ''}", r, m, ce_ref(out, sel, aux, lab, 8.0, hard), hard)


# ------------------------------------------------------------------ the data-parallel contract
@pytest.mark.parametrize("hard", [False, True])
def test_selective_and_bce_two_unequal_parts(hard):
    """Two ranks' parts of P_A and P_B pixels: partials per part, the fp64 sums added (the all-reduce), one finalize
    with p_global = P_A + P_B, bwd on part a with the shared state — the slice of the fp64 gradient of the loss
    over the concatenation."""
    pg = P_A + P_B
    o, s, t = b_inputs(pg, 3, seed=1)
    ref = b_ref(o, s, t, 8.0, hard)
    a, b = BForm(o[:P_A], s[:P_A], t[:P_A]), BForm(o[P_A:], s[P_A:], t[P_A:])
    sums = reduce_rows(a.partials(hard), 2) + reduce_rows(b.partials(hard), 2)
    loss, cov, state = selective_finalize(sums, pg, 8.0)
    assert state.cpu().tolist()[3] == float(pg)
    msum = reduce_rows(a.mean_partials(), 1) + reduce_rows(b.mean_partials(), 1)
    for part, sl in ((a, slice(0, P_A)), (b, slice(P_A, pg))):
        go, gs = part.bwd(state, 8.0, hard)
        r = dict(loss=loss.item(), cov=cov.item(), go=go, gs=gs)
        m = dict(loss=mean_finalize(msum, pg).item(), g=part.mean_bwd(pg))
        sub = (ref[0], ref[1], ref[2][sl], None if hard else ref[3][sl], ref[4], ref[5][sl])
        # (relative to the whole gradient's maximum, as one rank's slice of it)
        scale_o, scale_a = np.abs(ref[2]).max(), np.abs(ref[5]).max()
        assert np.abs(go.numpy() - sub[2]).max() <= TOL * scale_o
        assert np.abs(m["g"].numpy() - sub[5]).max() <= TOL * scale_a
        if not hard:
            assert np.abs(gs.numpy() - sub[3]).max() <= TOL * np.abs(ref[3]).max()
        check_b(f"two parts P={part.p}{' hard' if hard else ''}", r, m, sub, hard)


def test_ce_two_unequal_parts():
    n_a, n_b, c, hw = 3, 2, 8, 1639
    out, sel, aux, lab = ce_inputs(n_a + n_b, c, hw, seed=8)
    ref = ce_ref(out, sel, aux, lab, 8.0)
    pg = (n_a + n_b) * hw
    a, b = CEForm(out[:n_a], sel[:n_a], lab[:n_a]), CEForm(out[n_a:], sel[n_a:], lab[n_a:])
    ma, mb = CEForm(aux[:n_a], sel[:n_a], lab[:n_a]), CEForm(aux[n_a:], sel[n_a:], lab[n_a:])
    sums = reduce_rows(a.partials(), 2) + reduce_rows(b.partials(), 2)
    loss, cov, state = selective_finalize(sums, pg, 8.0)
    msum = reduce_rows(ma.mean_partials(), 1) + reduce_rows(mb.mean_partials(), 1)
    for part, mpart, sl in ((a, ma, slice(0, n_a)), (b, mb, slice(n_a, n_a + n_b))):
        go, gs = part.bwd(state, 8.0)
        r = dict(loss=loss.item(), cov=cov.item(), go=go, gs=gs)
        m = dict(loss=mean_finalize(msum, pg).item(), g=mpart.mean_bwd(pg))
        for got, k in ((go, 2), (gs, 3), (m["g"], 5)):
            assert np.abs(got.numpy() - ref[k][sl]).max() < CE_GRAD * np.abs(ref[k]).max()
        check_ce(f"ce two parts n={part.n}", r, m, (ref[0], ref[1], ref[2][sl], ref[3][sl], ref[4], ref[5][sl]), False)


# ------------------------------------------------------------------ upstream gradients
@pytest.mark.parametrize("sel_mean", [6.0, -3.0])
def test_selective_upstream_gradients(sel_mean):
    """g_loss = 0.5 and g_coverage = -0.25 (the fp64 gradient of 0.5 loss - 0.25 coverage), and null pointers
    (1 and 0). sel_mean = -3: coverage below the target, so d > 0 and the coverage term of d_sel is live;
    sel_mean = 6: coverage above it, d = 0."""
    p = P_A
    o, s, t = b_inputs(p, 3, sel_mean=sel_mean, seed=2)
    form = BForm(o, s, t)
    gl, gc = dev(np.float32([0.5])), dev(np.float32([-0.25]))
    for ups in (True, False):
        r = run_selective(form, 8.0, False, gl=gl if ups else None, gc=gc if ups else None)
        m = run_mean(form, gl=gl if ups else None)
        assert (r["state"][2].item() > 0) == (sel_mean < 0) == (r["cov"] < TC)
        ref = list(b_ref(o, s, t, 8.0, False, *((0.5, -0.25) if ups else (1.0, 0.0))))
        if ups:
            ref[5] = 0.5 * ref[5]
        check_b(f"upstream {'0.5/-0.25' if ups else 'null'} sel_mean={sel_mean}", r, m, ref, False)
    rh = run_selective(form, 8.0, True, gl=gl)  # hard: g_loss only (the coverage is detached)
    check_b(f"upstream hard sel_mean={sel_mean}", rh, m, b_ref(o, s, t, 8.0, True, 0.5, 0.0), True)


@pytest.mark.parametrize("sel_mean", [6.0, -3.0])
def test_ce_upstream_gradients(sel_mean):
    n, c, hw = CE_SHAPES[0]
    out, sel, aux, lab = ce_inputs(n, c, hw, sel_mean=sel_mean, seed=9)
    form, mform = CEForm(out, sel, lab), CEForm(aux, sel, lab)
    gl, gc = dev(np.float32([0.5])), dev(np.float32([-0.25]))
    for ups in (True, False):
        r = run_selective(form, 8.0, False, gl=gl if ups else None, gc=gc if ups else None)
        m = run_mean(mform, gl=gl if ups else None)
        assert (r["state"][2].item() > 0) == (sel_mean < 0) == (r["cov"] < TC)
        ref = list(ce_ref(out, sel, aux, lab, 8.0, False, *((0.5, -0.25) if ups else (1.0, 0.0))))
        if ups:
            ref[5] = 0.5 * ref[5]
        check_ce(f"ce upstream {'0.5/-0.25' if ups else 'null'} sel_mean={sel_mean}", r, m, ref, False)
