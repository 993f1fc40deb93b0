"""Connected regions of a label map and the cleanup of small ones (fcn8s_op_regions_label / fcn8s_op_regions_clean; the definition is in
include/fcn8s_hip.h).

An argmax map is full of specks -- a dozen "truck" pixels inside a car, a few "rider" pixels on a wall.  The usual remedy is to find the
connected components of the map and to merge the small ones into a neighbour.  The definition, per image L[H, W] with pixel index
i = y * W + x:

  * a component is a maximal set of pixels of equal class connected under `connectivity` (4 or 8); its id is the smallest pixel index it
    contains; comp[p] = the id, area[p] = the pixel count of p's component, both stored at every pixel;
  * a component of class c is small when area < min_area[c] (0: never small);
  * one round: for a small component S, every pair (p in S, q 4-adjacent to p, q not in S) whose q lies in a component T that is not small
    makes T a candidate; S takes the class of the candidate with the largest area, the smaller id on equal areas; without a candidate S
    keeps its class.  All decisions are taken on the round's input and applied together;
  * `rounds` rounds run back to back; per round the stats are (components, small components, relabelled components, pixels changed).

This module holds the NumPy restatement (`components_numpy`, `clean_numpy`: no SciPy, vectorised hooking and pointer jumping), the
resolution of the facade's `min_region` argument (`resolve`) and the calls on device tensors (`label_device`, `clean_device`).
"""
from __future__ import annotations

import numbers

import numpy as np

MAX_ROUNDS = 8
_LOW = np.uint64(0xFFFFFFFF)


def _check(connectivity, rounds=1):
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8, got %r" % (connectivity,))
    if isinstance(rounds, bool) or not isinstance(rounds, numbers.Integral) or not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError("rounds is an integer in 1..%d, got %r" % (MAX_ROUNDS, rounds))


def resolve(min_region, num_classes):
    """The facade's `min_region` as the 256-entry int32 table of thresholds, or None for "off".  An int: that threshold for every class
    below `num_classes`; a sequence of `num_classes` ints; a dict {class: area} (missing classes 0 = never small); None / 0 / False, or
    thresholds that are all 0: off.  Negative or non-integer values raise ValueError."""
    if min_region is None or min_region is False:
        return None
    num_classes = int(num_classes)
    if not 1 <= num_classes <= 256:
        raise ValueError("num_classes has to be in 1..256, got %d" % num_classes)

    def area(v):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("a region threshold is a non-negative integer, got %r" % (v,))
        if v < 0 or v >= 2 ** 31:
            raise ValueError("a region threshold is a non-negative integer below 2^31, got %r" % (v,))
        return int(v)

    table = np.zeros(256, np.int32)
    if isinstance(min_region, dict):
        for c, v in min_region.items():
            if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= c < num_classes:
                raise ValueError("min_region names class %r; the model has classes 0..%d" % (c, num_classes - 1))
            table[int(c)] = area(v)
    elif isinstance(min_region, (str, bytes)):
        raise ValueError("min_region is an int, a sequence of %d ints or a dict {class: area}, got %r" % (num_classes, min_region))
    elif isinstance(min_region, numbers.Number) or isinstance(min_region, np.generic):
        table[:num_classes] = area(min_region)
    else:
        try:
            seq = list(min_region)
        except TypeError:
            raise ValueError("min_region is an int, a sequence of %d ints or a dict {class: area}, got %r" % (num_classes, min_region))
        if len(seq) != num_classes:
            raise ValueError("min_region has %d entries; the model has %d classes" % (len(seq), num_classes))
        table[:num_classes] = [area(v) for v in seq]
    return table if table.any() else None


# ---- the NumPy restatement -------------------------------------------------------------------------------------------------------------
def _pairs(L, connectivity):
    """The index pairs (p, q) of adjacent pixels of equal class in one image (each unordered pair once)."""
    H, W = L.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    ok = (L >= 0) & (L < 256)
    out = []
    shifts = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    for dy, dx in shifts:
        if dx >= 0:
            a, b = (slice(0, H - dy), slice(0, W - dx)), (slice(dy, H), slice(dx, W))
        else:
            a, b = (slice(0, H - dy), slice(-dx, W)), (slice(dy, H), slice(0, W + dx))
        same = (L[a] == L[b]) & ok[a]
        out.append((idx[a][same], idx[b][same]))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _components_one(L, connectivity):
    H, W = L.shape
    lab = np.arange(H * W, dtype=np.int64)
    p, q = _pairs(L, connectivity)
    while p.size:
        a, b = lab[p], lab[q]
        m = np.minimum(a, b)
        np.minimum.at(lab, a, m)                  # hook the larger representative below the smaller (a representative only ever falls)
        np.minimum.at(lab, b, m)
        while True:                               # pointer jumping to the roots
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        keep = lab[p] != lab[q]
        p, q = p[keep], q[keep]
    area = np.bincount(lab, minlength=H * W)[lab]
    return lab.reshape(H, W).astype(np.int32), area.reshape(H, W).astype(np.int32)


def _as_maps(L):
    L = np.asarray(L)
    if L.ndim not in (2, 3) or L.dtype.kind not in "iu":
        raise ValueError("a label map is an integer array [H, W] or [N, H, W], got %s %s" % (L.dtype, L.shape))
    return L


def components_numpy(L, connectivity=4):
    """(comp, area), int32 arrays of L's shape ([H, W] or [N, H, W]): the id and the pixel count of every pixel's component."""
    _check(connectivity)
    L = _as_maps(L)
    if L.ndim == 2:
        return _components_one(L.astype(np.int64), connectivity)
    res = [_components_one(x.astype(np.int64), connectivity) for x in L]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _table(min_area):
    if isinstance(min_area, numbers.Integral) and not isinstance(min_area, bool):
        return np.full(256, int(min_area), np.int64)
    t = np.asarray(min_area)
    if t.shape != (256,) or t.dtype.kind not in "iu":
        raise ValueError("min_area is an int or a table of 256 integers")
    return t.astype(np.int64)


def _clean_round(L, table, connectivity):
    H, W = L.shape
    comp, area = _components_one(L, connectivity)
    comp = comp.astype(np.int64).ravel(); area = area.astype(np.int64).ravel()
    flat = L.ravel()
    ok = (flat >= 0) & (flat < 256)
    thr = np.where(ok, table[np.where(ok, flat, 0)], 0)
    small = ok & (thr > 0) & (area < thr)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    best = np.zeros(H * W, np.uint64)
    for a, b in (((slice(0, H), slice(0, W - 1)), (slice(0, H), slice(1, W))), ((slice(0, H - 1), slice(0, W)), (slice(1, H), slice(0, W)))):
        for p, q in ((idx[a].ravel(), idx[b].ravel()), (idx[b].ravel(), idx[a].ravel())):
            use = small[p] & ~small[q] & ok[q]
            p, q = p[use], q[use]
            key = (area[q].astype(np.uint64) << np.uint64(32)) | (_LOW - comp[q].astype(np.uint64))
            np.maximum.at(best, comp[p], key)
    won = best[comp]
    has = small & (won > 0)
    winner = (_LOW - (won & _LOW)).astype(np.int64)
    out = np.where(has, flat[np.where(has, winner, 0)], flat).reshape(H, W)
    roots = comp == idx.ravel()
    stats = [int(roots.sum()), int((roots & small).sum()), int((roots & has).sum()), int(has.sum())]
    return out, stats


def clean_numpy(L, min_area, connectivity=4, rounds=1):
    """(L', stats): the map after `rounds` rounds of cleanup (L's shape and dtype) and the int64 [rounds, 4] stats, summed over the images
    of a stack.  `min_area`: an int (every class) or a table of 256 ints."""
    _check(connectivity, rounds)
    L = _as_maps(L)
    table = _table(min_area)
    maps = [L] if L.ndim == 2 else list(L)
    stats = np.zeros((rounds, 4), np.int64)
    outs = []
    for x in maps:
        x = x.astype(np.int64)
        for r in range(rounds):
            x, st = _clean_round(x, table, connectivity)
            stats[r] += st
        outs.append(x.astype(L.dtype))
    return (outs[0] if L.ndim == 2 else np.stack(outs)), stats


# ---- the calls on device tensors -----------------------------------------------------------------------------------------------------------
def _kind(labels):
    import torch
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise ValueError("labels have to be a tensor on the GPU")
    if labels.dtype == torch.int64:
        kind = 0
    elif labels.dtype == torch.uint8:
        kind = 1
    else:
        raise ValueError("labels are int64 (as `predict` returns them) or uint8, got %s" % labels.dtype)
    if labels.dim() not in (2, 3) or not labels.is_contiguous():
        raise ValueError("labels are a contiguous tensor [H, W] or [N, H, W]")
    N, H, W = (1,) + tuple(labels.shape) if labels.dim() == 2 else tuple(labels.shape)
    return kind, int(N), int(H), int(W)


def work_bytes(N, H, W):
    from . import _lib as L
    n = int(L.lib.fcn8s_op_regions_work_bytes(int(N), int(H), int(W)))
    if n == 0:
        raise ValueError("regions: N, H, W have to be positive and H * W below 2^31, got %r" % ((N, H, W),))
    return n


def _work(work, nbytes, device):
    import torch
    if work is None or work.numel() < nbytes:
        work = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return work


def label_device(labels, connectivity=4, area=True, work=None):
    """One `fcn8s_op_regions_label` call on a device tensor (int64 or uint8, [H, W] or [N, H, W]): (comp, area | None, work), int32 device
    tensors of the labels' shape.  `work`: a uint8 device tensor to reuse (a larger one is made when it is too small) -- returned."""
    import ctypes as C
    import torch
    from . import _lib as L
    _check(connectivity)
    kind, N, H, W = _kind(labels)
    work = _work(work, 256, labels.device)
    comp = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    ar = torch.empty(labels.shape, dtype=torch.int32, device=labels.device) if area else None
    stream = C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)
    L.check(L.lib.fcn8s_op_regions_label(stream, C.c_void_p(labels.data_ptr()), kind, N, H, W, int(connectivity), C.c_void_p(comp.data_ptr()),
                                         C.c_void_p(ar.data_ptr()) if area else None, C.c_void_p(work.data_ptr())))
    return comp, ar, work


def clean_device(labels, min_area, connectivity=4, rounds=1, stats=False, work=None):
    """One `fcn8s_op_regions_clean` call, in place, on a device tensor (int64 or uint8, [H, W] or [N, H, W]).  `min_area`: an int, a table of
    256 ints, or an int32 device tensor of 256.  Returns (stats | None, work): the int64 [rounds, 4] stats as a device tensor when asked for."""
    import ctypes as C
    import torch
    from . import _lib as L
    _check(connectivity, rounds)
    kind, N, H, W = _kind(labels)
    if isinstance(min_area, torch.Tensor):
        if min_area.dtype != torch.int32 or min_area.numel() != 256 or not min_area.is_cuda or not min_area.is_contiguous():
            raise ValueError("a min_area tensor is 256 contiguous int32 on the GPU")
        table = min_area
    else:
        t = _table(min_area)
        if t.min() < 0 or t.max() >= 2 ** 31:
            raise ValueError("region thresholds are non-negative and below 2^31")
        table = torch.from_numpy(t.astype(np.int32)).to(labels.device)
    work = _work(work, work_bytes(N, H, W), labels.device)
    st = torch.empty((rounds, 4), dtype=torch.int64, device=labels.device) if stats else None
    stream = C.c_void_p(torch.cuda.current_stream(labels.device).cuda_stream)
    L.check(L.lib.fcn8s_op_regions_clean(stream, C.c_void_p(labels.data_ptr()), kind, N, H, W, int(connectivity), C.c_void_p(table.data_ptr()),
                                         int(rounds), C.c_void_p(work.data_ptr()), C.c_void_p(st.data_ptr()) if stats else None))
    return st, work


def status_device(work):
    """(flag bits, pixels with a label out of range) of the most recent label / clean call on `work`; synchronises.  Flag bits other than 0
    mean that a bounded loop of the union-find gave up (never seen): the result of that call is not to be trusted."""
    import ctypes as C
    import torch
    from . import _lib as L
    out = (C.c_int64 * 2)()
    stream = C.c_void_p(torch.cuda.current_stream(work.device).cuda_stream)
    L.check(L.lib.fcn8s_op_regions_status(stream, C.c_void_p(work.data_ptr()), out))
    return int(out[0]), int(out[1])
