"""The training augmentation without a GPU: the glass table, the counter hash, the colour table,
the loader's plan and the argument checks. The kernel itself is in tests/test_gpu_augment.py."""
import numpy as np
import pytest
import torch

from selectivenet_for_semantic_segmentation_binary_amd import data as D
from selectivenet_for_semantic_segmentation_binary_amd.train import parse_arguments
from tests import _augment_ref as AR
from tests import _tissue_ref as TS


# ----------------------------------------------------------------------------- the glass table
def test_glass_table_is_the_quantised_glass_model():
    T = D.glass_table()
    assert T.dtype == np.uint8 and T.shape == (4096,)
    assert np.array_equal(T, AR.glass_table())
    assert (np.diff(T.astype(int)) >= 0).all()
    assert T.min() >= 237 and int(T.max()) - int(T.min()) <= 11
    assert (int(T.min()), int(T.max())) == (240, 249)
    print(f"mean {T.mean():.4f} std {T.std():.4f}")
    assert abs(T.mean() - 244.8) <= 0.05 and 1.25 <= T.std() <= 1.35
    assert D.glass_table() is T  # built once


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_painted_quadrant_is_glass_under_predicts_default_rule(q):
    """Every painted pixel is glass for predict --tissue's defaults (tests/_tissue_ref.py's pixel rule), and a dark
    patch stays tissue outside the quadrant."""
    h, w = 14, 20
    img = np.full((1, h, w, 3), 90, np.uint8)
    lab = np.full((1, h, w), 255, np.uint8)
    oi, ol = AR.augment_bytes(img, lab, glass=[q], keys=[1234567 * q])
    m = AR.quadrant_mask(h, w, q)
    assert m.sum() == (h // 2) * (w // 2)
    plane = TS.plane_of(oi[0])
    assert (plane[m] == 0).all() and (plane[~m] == 255).all()
    assert (ol[0][m] == 0).all() and (ol[0][~m] == 255).all()


# ----------------------------------------------------------------------------- the hash
@pytest.mark.parametrize("key", [0, 1, 0xDEADBEEF])
def test_hash_drives_the_table_like_uniform_noise(key):
    """2^20 consecutive counters: the mean of T[u >> 20] within 6 standard errors of mean(T), and the lag-1 and
    lag-3 correlations (neighbouring channels, neighbouring pixels) within 6 / sqrt(N)."""
    T = AR.glass_table().astype(np.float64)
    N = 1 << 20
    v = T[AR.u(key, np.arange(N, dtype=np.uint32)) >> np.uint32(20)]
    z = abs(v.mean() - T.mean()) / (T.std() / np.sqrt(N))
    d = v - v.mean()
    r = [abs(float((d[:-lag] * d[lag:]).sum() / (d * d).sum())) * np.sqrt(N) for lag in (1, 3)]
    print(f"key {key:#x}: mean z {z:.2f}, |r| sqrt(N) at lags 1, 3: {r[0]:.2f} {r[1]:.2f}")
    assert z <= 6 and max(r) <= 6


def test_hash_depends_on_key_and_counter_only():
    a = AR.u(7, np.arange(64, dtype=np.uint32))
    assert np.array_equal(a, AR.u(7, np.arange(64, dtype=np.uint32)))
    assert not np.array_equal(a, AR.u(8, np.arange(64, dtype=np.uint32)))
    assert len(set(a.tolist())) == 64
    # a value worked by hand in Python integers
    M = 0xFFFFFFFF

    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & M
        x ^= x >> 15
        x = x * 0x846CA68B & M
        return x ^ x >> 16

    for key, c in ((0, 0), (7, 5), (0xFFFFFFFF, 0xFFFFFFFF), (123456789, 3 * 1000003)):
        assert int(AR.u(key, c)[0]) == mix((mix(key) + c * 0x9E3779B9) & M)


# ----------------------------------------------------------------------------- the colour table
def test_color_lut():
    one, zero = np.ones((2, 3)), np.zeros((2, 3))
    ident = D.color_lut(one, zero)
    assert ident.dtype == np.uint8 and ident.shape == (2, 3, 256)
    assert np.array_equal(ident, np.broadcast_to(np.arange(256, dtype=np.uint8), (2, 3, 256)))
    rng = np.random.Generator(np.random.PCG64(5))
    gamma, beta = rng.uniform(0.5, 1.5, (200, 3)), rng.uniform(-0.5, 0.5, (200, 3))
    gamma[0], beta[0] = 0.5, -0.5   # the corners of sigma = 0.5
    gamma[1], beta[1] = 1.5, 0.5
    gamma[2], beta[2] = 0.5, 0.5
    gamma[3], beta[3] = 1.5, -0.5
    lut = D.color_lut(gamma, beta)
    assert np.array_equal(lut, AR.color_lut(gamma, beta))
    assert (np.diff(lut.astype(int), axis=-1) >= 0).all()
    assert (lut[..., 0] == 0).all()
    assert lut[0].max() == 255 and (lut[1][..., 255] == int(np.floor(255 * np.exp(-0.5) + 0.5))).all()
    for bad in ((np.ones((2, 2)), np.zeros((2, 2))), (np.ones((2, 3)), np.zeros((3, 3))), (np.ones(3), np.zeros(3)),
                (np.zeros((1, 3)), np.zeros((1, 3))), (np.full((1, 3), np.nan), np.zeros((1, 3)))):
        with pytest.raises(ValueError):
            D.color_lut(*bad)


# ----------------------------------------------------------------------------- the plan
N_DS = 45


def loader(seed=7, epoch=3, bs=16, n=N_DS, **aug):
    ds = D.PatchSet(np.zeros((n, 8, 8, 3), np.uint8), np.zeros((n, 8, 8), np.uint8))
    ld = D.BatchLoader(ds, bs, shuffle=True, random_flip=True, device="cpu", seed=seed, **aug)
    ld.set_epoch(epoch)
    return ld


ALL = dict(aug_d4=True, aug_glass=0.25, aug_color=0.3)


def rows_of(plan):
    """The plan flattened: {field: array over the epoch's images in plan order}."""
    out = {"idx": np.concatenate([p[1] for p in plan]), "fl": np.concatenate([p[2] for p in plan])}
    if len(plan[0]) > 3:
        for f in D.AugRows._fields:
            if getattr(plan[0][3], f) is not None:
                out[f] = np.concatenate([getattr(p[3], f) for p in plan])
    return out


@pytest.mark.parametrize("aug", [dict(aug_d4=True), dict(aug_glass=0.25), dict(aug_color=0.3), ALL])
def test_plan_keeps_order_and_flips_with_any_option(aug):
    base, plan = loader()._plan(), loader(**aug)._plan()
    assert all(len(p) == 3 for p in base) and all(len(p) == 4 for p in plan) and len(base) == len(plan)
    for p0, p1 in zip(base, plan):
        assert p0[0] == p1[0] and np.array_equal(p0[1], p1[1]) and np.array_equal(p0[2], p1[2])
        assert np.array_equal(p1[3].geom & 3, p0[2]) and p1[3].geom.dtype == np.uint8
        assert ((p1[3].geom & 4) == 0).all() or aug.get("aug_d4")
        assert (p1[3].glass is None) == (p1[3].key is None) == ("aug_glass" not in aug)
        assert (p1[3].gamma is None) == (p1[3].beta is None) == ("aug_color" not in aug)


def test_each_options_draws_are_unchanged_by_the_others():
    every = rows_of(loader(**ALL)._plan())
    d4 = rows_of(loader(aug_d4=True)._plan())
    gl = rows_of(loader(aug_glass=0.25)._plan())
    co = rows_of(loader(aug_color=0.3)._plan())
    assert np.array_equal(d4["geom"], every["geom"]) and (every["geom"] & 4).any() and not (every["geom"] & 4).all()
    assert np.array_equal(gl["glass"], every["glass"]) and np.array_equal(gl["key"], every["key"])
    assert gl["key"].dtype == np.uint32 and len(set(gl["key"].tolist())) == N_DS
    assert np.array_equal(co["gamma"], every["gamma"]) and np.array_equal(co["beta"], every["beta"])
    assert co["gamma"].shape == (N_DS, 3) and co["gamma"].dtype == np.float64
    assert (np.abs(co["gamma"] - 1) <= 0.3).all() and (np.abs(co["beta"]) <= 0.3).all()
    assert np.abs(co["gamma"] - 1).max() > 0.2 and np.abs(co["beta"]).max() > 0.2
    # a larger sigma scales the same uniforms; a larger P paints a superset with the same quadrants
    co2 = rows_of(loader(aug_color=0.15)._plan())
    assert np.allclose(co2["gamma"] - 1, (co["gamma"] - 1) / 2, atol=1e-15)
    gl2 = rows_of(loader(aug_glass=0.75)._plan())
    painted = gl["glass"] != 0
    assert np.array_equal(gl2["glass"][painted], gl["glass"][painted]) and (gl2["glass"] != 0).sum() > painted.sum()


def test_draws_are_per_dataset_index():
    """The same image has the same augmentation wherever the shuffle and the batch size put it."""
    a, b = rows_of(loader(**ALL)._plan()), rows_of(loader(bs=7, **ALL)._plan())
    ia, ib = np.argsort(a["idx"]), np.argsort(b["idx"])
    for f in ("geom", "glass", "key", "gamma", "beta"):
        assert np.array_equal(a[f][ia], b[f][ib]), f


def test_plan_chunks_of_two_ranks_are_the_single_ranks(monkeypatch):
    one = loader(**ALL)._plan()
    chunks = []
    for r in range(2):
        monkeypatch.setattr(D.parallel, "world_size", lambda: 2)
        monkeypatch.setattr(D.parallel, "rank", lambda r=r: r)
        chunks.append(loader(**ALL)._plan())
    assert len(chunks[0]) == len(chunks[1]) == len(one)
    for p, c0, c1 in zip(one, chunks[0], chunks[1]):
        assert c0[0] == c1[0] == p[0] and len(c0[1]) > 0 and len(c1[1]) > 0
        assert np.array_equal(np.concatenate([c0[1], c1[1]]), p[1])
        assert np.array_equal(np.concatenate([c0[2], c1[2]]), p[2])
        for f in D.AugRows._fields:
            assert np.array_equal(np.concatenate([getattr(c0[3], f), getattr(c1[3], f)]), getattr(p[3], f)), f


def test_plan_changes_with_the_epoch_and_the_seed():
    a = rows_of(loader(**ALL)._plan())
    assert all(np.array_equal(v, rows_of(loader(**ALL)._plan())[k]) for k, v in a.items())
    for other in (loader(epoch=4, **ALL), loader(seed=8, **ALL)):
        b = rows_of(other._plan())
        ia, ib = np.argsort(a["idx"]), np.argsort(b["idx"])
        for f in ("geom", "glass", "key", "gamma"):
            assert not np.array_equal(a[f][ia], b[f][ib]), f


def test_glass_share_and_quadrants():
    n, p = 10_000, 0.25
    ld = loader(n=n, bs=500, aug_glass=p)
    g = rows_of(ld._plan())["glass"]
    share = (g != 0).mean()
    print(f"glass share {share:.4f}; quadrants {np.bincount(g, minlength=5)[1:]}")
    assert abs(share - p) <= 6 * np.sqrt(p * (1 - p) / n)
    assert set(g.tolist()) == {0, 1, 2, 3, 4}
    counts = np.bincount(g, minlength=5)[1:]
    assert (np.abs(counts - counts.sum() / 4) <= 6 * np.sqrt(counts.sum() * 3 / 16)).all()
    assert (rows_of(loader(n=200, bs=50, aug_glass=1.0)._plan())["glass"] != 0).all()


def test_default_loader_is_todays(monkeypatch):
    """No option set: three-element plan items, three uploads (images, labels, flips), no augmentation state.
    (Pinning needs a device: here the host tensors stay pageable.)"""
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    ld = loader()
    assert not ld.aug
    item = ld._plan()[0]
    gb, host, transposed = ld._host(item)
    assert len(host) == 3 and transposed is False and np.array_equal(host[2].numpy(), item[2])
    ld2 = loader(**ALL)
    gb, host, transposed = ld2._host(ld2._plan()[0])
    a = ld2._plan()[0][3]
    assert len(host) == 6 and transposed == bool((a.geom & 4).any())
    assert host[4].dtype == torch.int32 and np.array_equal(host[4].numpy().view(np.uint32), a.key)
    assert np.array_equal(host[5].numpy(), AR.color_lut(a.gamma, a.beta))


# ----------------------------------------------------------------------------- arguments
def test_loader_argument_checks():
    for bad in (dict(aug_glass=-0.1), dict(aug_glass=1.5), dict(aug_glass=float("nan")), dict(aug_color=-0.1),
                dict(aug_color=0.6), dict(aug_color=float("nan"))):
        with pytest.raises(ValueError):
            loader(**bad)
    ds = D.PatchSet(np.zeros((4, 8, 16, 3), np.uint8), np.zeros((4, 8, 16), np.uint8))
    with pytest.raises(ValueError, match="square"):
        D.BatchLoader(ds, 2, shuffle=True, random_flip=True, device="cpu", aug_d4=True)
    D.BatchLoader(ds, 2, shuffle=True, random_flip=True, device="cpu", aug_glass=0.5, aug_color=0.1)


def test_prep_batch_aug_argument_checks_before_any_launch():
    img, lab = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    geom = torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="input_type"):
        D.prep_batch_aug(img, lab, geom, input_type="HSV")
    with pytest.raises(RuntimeError, match="images must be a contiguous cuda uint8"):
        D.prep_batch_aug(img, lab, geom)


def test_cli_options(capsys):
    a = parse_arguments([])
    assert (a.aug_d4, a.aug_glass, a.aug_color) == (0, 0.0, 0.0)
    a = parse_arguments("--aug_d4 1 --aug_glass 0.25 --aug_color 0.1".split())
    assert (a.aug_d4, a.aug_glass, a.aug_color) == (1, 0.25, 0.1)
    parse_arguments("--aug_glass 1 --aug_color 0.5".split())
    for bad in ("--aug_d4 2", "--aug_glass -0.01", "--aug_glass 1.01", "--aug_glass nan", "--aug_color -0.1",
                "--aug_color 0.51", "--aug_color nan"):
        with pytest.raises(SystemExit):
            parse_arguments(bad.split())
    assert "aug_" in capsys.readouterr().err
