"""Flip / D4 test-time augmentation restated in numpy (test infrastructure), on top of tests/_predict_ref.py:
the eight maps T_k and their inverses, the fixed-order fp32 reduction of the members, the votes and the mask
rule — around whatever plain prediction the caller passes (the tiled CPU oracle in tests/test_tta_host.py,
`predict_image` on the GPU in tests/test_gpu_predict_tta.py). Written from DESIGN.md §7g, not from predict.py."""
from __future__ import annotations

import numpy as np

F32 = np.float32
MEMBERS = {"flips": 4, "d4": 8}


def T(k, img):
    """Member k's view of an [H,W] or [H,W,C] array: bit 2 transposes, then bit 1 flips the rows, then bit 0
    the columns."""
    m = img
    if k & 4:
        m = np.swapaxes(m, 0, 1)
    if k & 2:
        m = m[::-1]
    if k & 1:
        m = m[:, ::-1]
    return m


def T_inv(k, p):
    """The inverse of T(k, .): the same steps undone in reverse order."""
    if k & 1:
        p = p[:, ::-1]
    if k & 2:
        p = p[::-1]
    if k & 4:
        p = np.swapaxes(p, 0, 1)
    return p


def member_planes(plain, image, members):
    """[(out_k, sel_k)] for k < members, each mapped back to the image's orientation: `plain(image_k)` ->
    (out, sel) fp32 [H_k,W_k] is today's prediction of the contiguous image T_k(image)."""
    res = []
    for k in range(members):
        out, sel = plain(np.array(T(k, image), order="C"))
        res.append((np.ascontiguousarray(T_inv(k, out)), None if sel is None else np.ascontiguousarray(T_inv(k, sel))))
    return res


def reduce_members(planes):
    """The mean of 4 or 8 fp32 planes in the pinned order: A = ((m0 + m1) + m2) + m3, B likewise over m4..m7
    (an elementwise sum is the same in either orientation), mean = A / 4 or (A + B) / 8."""
    assert len(planes) in (4, 8) and all(p.dtype == F32 for p in planes)
    with np.errstate(invalid="ignore", over="ignore"):
        A = ((planes[0] + planes[1]) + planes[2]) + planes[3]
        if len(planes) == 4:
            return A * F32(0.25)
        B = ((planes[4] + planes[5]) + planes[6]) + planes[7]
        return (A + B) * F32(0.125)


def votes_of(planes, t):
    """uint8: the number of members with plane >= t (a NaN casts no vote)."""
    with np.errstate(invalid="ignore"):
        return sum((p >= F32(t)).astype(np.uint8) for p in planes)


def mask_of(out, sel, t_out, t_sel):
    """0 background, 127 abstained, 255 tumor: `not (sel >= t_sel)` abstains (so a NaN does), a NaN output is
    background. sel None: no selection head."""
    with np.errstate(invalid="ignore"):
        m = np.where(out >= F32(t_out), 255, 0)
        if sel is not None:
            m = np.where(~(sel >= F32(t_sel)), 127, m)
    return m.astype(np.uint8)


def counts_of(mask):
    return [int((mask == 0).sum()), int((mask == 255).sum()), int((mask == 127).sum()), int(mask.size)]


def tta_ref(plain, image, members, t_out, t_sel):
    """§7g as a whole: {"logit", "selection", "mask", "votes", "sel_votes", "counts", "members"}."""
    mem = member_planes(plain, image, members)
    outs = [m[0] for m in mem]
    sels = None if mem[0][1] is None else [m[1] for m in mem]
    logit = reduce_members(outs)
    selection = None if sels is None else reduce_members(sels)
    mask = mask_of(logit, selection, t_out, t_sel)
    return {"logit": logit, "selection": selection, "mask": mask, "votes": votes_of(outs, t_out),
            "sel_votes": None if sels is None else votes_of(sels, t_sel), "counts": counts_of(mask), "members": mem}
