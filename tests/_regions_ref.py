"""Connected regions, their table and the two clean-up steps restated in plain numpy / Python (test
infrastructure), from the definitions in DESIGN.md §7h, not from predict.py or the kernels: a breadth-first
flood fill started at every unlabelled pixel in raster order, so a region's label 1 + y W + x is that of its
first pixel by construction."""
from __future__ import annotations

from collections import deque

import numpy as np

COLUMNS = ("label", "area", "y_min", "x_min", "y_max", "x_max", "sum_y", "sum_x", "prob_sum", "abstain_contacts")
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def label(mask, value=255, connectivity=8):
    """int32 [H,W]: 1 + y W + x of the first pixel (raster order) of the pixel's region of `value`; 0 elsewhere."""
    assert connectivity in (4, 8)
    mask = np.asarray(mask)
    H, W = mask.shape
    hit = (mask == value).tolist()
    lab = [[0] * W for _ in range(H)]
    nb = N8 if connectivity == 8 else N4
    for y in range(H):
        row = hit[y]
        for x in range(W):
            if not row[x] or lab[y][x]:
                continue
            name = 1 + y * W + x
            lab[y][x] = name
            todo = deque([(y, x)])
            while todo:
                cy, cx = todo.popleft()
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and hit[ny][nx] and not lab[ny][nx]:
                        lab[ny][nx] = name
                        todo.append((ny, nx))
    return np.array(lab, np.int32).reshape(H, W)


def table(mask, labels, prob8=None):
    """{column: int64 [n]}, rows ascending by label; prob_sum only with prob8."""
    mask, labels = np.asarray(mask), np.asarray(labels)
    H, W = mask.shape
    ab = np.pad(mask == 127, 1)  # outside the image: no neighbour
    contacts = (ab[:-2, 1:-1].astype(np.int64) + ab[2:, 1:-1] + ab[1:-1, :-2] + ab[1:-1, 2:])
    ys, xs = np.nonzero(labels > 0)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    names, row = np.unique(labels[ys, xs], return_inverse=True)  # ascending; row: each pixel's region
    n = len(names)

    def total(values):  # exact integer sums per region
        acc = np.zeros(n, np.int64)
        np.add.at(acc, row, values)
        return acc

    def extreme(values, ufunc, start):
        acc = np.full(n, start, np.int64)
        ufunc.at(acc, row, values)
        return acc

    out = {"label": names.astype(np.int64), "area": total(np.ones_like(ys)),
           "y_min": extreme(ys, np.minimum, H), "x_min": extreme(xs, np.minimum, W),
           "y_max": extreme(ys, np.maximum, -1), "x_max": extreme(xs, np.maximum, -1),
           "sum_y": total(ys), "sum_x": total(xs)}
    if prob8 is not None:
        out["prob_sum"] = total(np.asarray(prob8)[ys, xs].astype(np.int64))
    out["abstain_contacts"] = total(contacts[ys, xs])
    return out


def counts(mask):
    mask = np.asarray(mask)
    c = [int((mask == v).sum()) for v in (0, 255, 127)]
    return c + [sum(c)]


def clean(mask, prob8=None, min_region=0, fill_holes=0, connectivity=8):
    """The two steps on a copy: (final mask, table of its 255-regions, counts, {removed_regions, removed_pixels,
    filled_holes, filled_pixels})."""
    m = np.array(mask, np.uint8)
    H, W = m.shape
    done = {"removed_regions": 0, "removed_pixels": 0, "filled_holes": 0, "filled_pixels": 0}
    if min_region > 0:
        lab = label(m, 255, connectivity)
        t = table(m, lab)
        small = t["area"] < min_region
        m[np.isin(lab, t["label"][small])] = 0
        done["removed_regions"], done["removed_pixels"] = int(small.sum()), int(t["area"][small].sum())
    if fill_holes > 0:
        lab = label(m, 0, 12 - connectivity)
        t = table(m, lab)
        inside = (t["y_min"] > 0) & (t["x_min"] > 0) & (t["y_max"] < H - 1) & (t["x_max"] < W - 1)
        hole = inside & (t["abstain_contacts"] == 0) & (t["area"] <= fill_holes)
        m[np.isin(lab, t["label"][hole])] = 255
        done["filled_holes"], done["filled_pixels"] = int(hole.sum()), int(t["area"][hole].sum())
    return m, table(m, label(m, 255, connectivity), prob8), counts(m), done


# ----------------------------------------------------------------------------- labels without a flood fill
ONE_PATH = ("spiral", "serpentine", "comb")  # a single region under either connectivity, (0, 0) its first pixel


def analytic_labels(name, mask, connectivity):
    """The labels of the 255-regions of pattern `name`, known without a search (tests/test_io_regimes_host.py holds
    them against label() at 70 x 130): (0, 0) is set in all four patterns; spiral, serpentine and comb are one
    region under 4 and under 8, the checkerboard is one region under 8 (every set pixel touches the next
    diagonally), and under 4 every set pixel of it is a region of its own, 1 + y W + x."""
    assert name in ONE_PATH + ("checkerboard",) and connectivity in (4, 8) and mask[0, 0] == 255
    H, W = mask.shape
    hit = mask == 255
    if name == "checkerboard" and connectivity == 4:
        own = 1 + np.arange(H, dtype=np.int64)[:, None] * W + np.arange(W, dtype=np.int64)[None, :]
        return np.where(hit, own, 0).astype(np.int32)
    return hit.astype(np.int32)


def canonical(lab):
    """Any labelling (0 = background, one positive integer per region, scipy.ndimage.label's for instance) renamed
    to 1 + the raster index of each region's first pixel."""
    lab = np.asarray(lab)
    flat = lab.reshape(-1)
    pos = np.flatnonzero(flat)
    names, first = np.unique(flat[pos], return_index=True)  # the first occurrence in raster order
    rename = np.zeros(int(flat.max()) + 1, np.int64)
    rename[names] = 1 + pos[first]
    return rename[flat].reshape(lab.shape).astype(np.int32)


# ----------------------------------------------------------------------------- patterns
def checkerboard(H, W):
    return (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0) * 255).astype(np.uint8)


def diagonals(H, W, step=64):
    """One-pixel-wide diagonals of both directions through the corners of step x step tiles."""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return ((((y - x) % step == 0) | ((y + x + 1) % step == 0)) * 255).astype(np.uint8)


def spiral(H, W):
    """A one-pixel-wide rectangular spiral with one-pixel gaps, from the outer border inwards."""
    m = np.zeros((H, W), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 255
    free = lambda yy, xx: 0 <= yy < H and 0 <= xx < W and m[yy, xx] == 0  # noqa: E731
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        # go on while the next pixel is free and the one after it is not part of the spiral already
        if free(ny, nx) and not (0 <= ahead[0] < H and 0 <= ahead[1] < W and m[ahead] == 255):
            y, x = ny, nx
            m[y, x] = 255
            turns = 0
        else:
            dy, dx = dx, -dy  # turn right
            turns += 1
    return m


def serpentine(H, W):
    """Every second row full, joined alternately at the right and the left end: one 4-connected path."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 255
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = 255
    return m


def comb(H, W):
    """Teeth in every second column that join only in the last row."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = 255
    m[H - 1] = 255
    return m


def noise(H, W, p, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((rng.random((H, W)) < p) * 255).astype(np.uint8)


def blobs(H, W, seed):
    """A three-valued mask: smooth random blobs of 255 and of 127 on 0."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def field():
        f = rng.normal(size=(H + 8, W + 8))
        for _ in range(3):  # a cheap smoothing: box sums along both axes
            f = f[:-1] + f[1:]
            f = f[:, :-1] + f[:, 1:]
        return f[:H, :W]

    a, b = field(), field()
    m = np.zeros((H, W), np.uint8)
    m[a > np.quantile(a, 0.6)] = 255
    m[b > np.quantile(b, 0.75)] = 127
    return m
