"""ClassMix self-training (Olsson et al., WACV 2021; the mixing of DACS, Tranheden et al., WACV 2021): the NumPy restatement of
`fcn8s_op_class_mix`, the validation of `FCN8s.train(unlabeled_generator=...)`'s arguments, and the device wrapper.

The definition is in include/fcn8s_hip.h at `fcn8s_op_class_mix`.  For destination image n with source s = src[n]: the classes below C that
occur in labels[s] are ranked by a Philox key of (draw, n, class), the ceil(k / 2) lowest ranks are selected, and wherever labels[s] holds a
selected class the pixel and its label come from s, elsewhere from n.  Everything is an integer; `mix_numpy` and the kernel agree with `==`."""
from __future__ import annotations

import numpy as np

STREAM = 0x434D4958          # the Philox stream of the selection keys ("CMIX")
MAX_CLASSES = 255
MAX_BATCH = 256
MAX_DRAW = 1 << 48
PREDICT_KEYS = ('scales', 'flip', 'crf', 'temperature', 'samples', 'keep_prob', 'mi_max')

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox_u32(idx, seed, stream):
    """The library's `philox_u32` (csrc/fcn8s_internal.h: Philox-4x32, ten rounds, the first output word) of a uint64 array of counters."""
    idx = np.asarray(idx, np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c0, c1 = idx & _LOW, idx >> _S32
    c2 = np.full(idx.shape, int(stream) & 0xFFFFFFFF, np.uint64)
    c3 = np.full(idx.shape, _W0, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                         # 32 x 32 -> 64 bits: no overflow
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LOW, n2, p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0.astype(np.uint32)


def _check_op(C, seed, draw):
    if not 2 <= int(C) <= MAX_CLASSES:
        raise ValueError("class mixing takes 2..{} classes, got {}".format(MAX_CLASSES, C))
    if not 0 <= int(draw) < MAX_DRAW:
        raise ValueError("`draw` must lie in [0, 2^48), got {!r}".format(draw))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("`seed` must lie in [0, 2^64), got {!r}".format(seed))


def select_classes(labels_s, C, seed, draw, n):
    """The 256-entry table (uint8, 1 = selected) of destination image `n` whose source has the label map `labels_s` (any shape)."""
    _check_op(C, seed, draw)
    C = int(C)
    present = np.bincount(np.asarray(labels_s, np.uint8).reshape(-1), minlength=256)[:C] > 0
    idx = np.uint64((int(draw) << 16) + (int(n) << 8)) + np.arange(C, dtype=np.uint64)
    keys = philox_u32(idx, seed, STREAM)
    order = np.lexsort((np.arange(C), keys))                # by key, then by class
    order = order[present[order]]
    out = np.zeros(256, np.uint8)
    out[order[:(len(order) + 1) // 2]] = 1
    return out


def mix_numpy(images, labels, src, C, seed, draw):
    """(images', labels', selected [N, 256]) as `fcn8s_op_class_mix` writes them: images uint8 [N, ..., 3], labels uint8 [N, ...], src N ints
    (one outside [0, N) counts as n, as in the kernel)."""
    images, labels = np.asarray(images), np.asarray(labels)
    if images.dtype != np.uint8 or labels.dtype != np.uint8 or images.shape != labels.shape + (3,) or labels.ndim < 2:
        raise ValueError("images are uint8 [N, ..., 3] and labels uint8 [N, ...] of the same pixels")
    N = labels.shape[0]
    src = np.asarray(src, np.int64).reshape(-1)
    if src.size != N:
        raise ValueError("`src` holds one source per image")
    out_i, out_l = images.copy(), labels.copy()
    selected = np.zeros((N, 256), np.uint8)
    for n in range(N):
        s = int(src[n]) if 0 <= src[n] < N else n
        selected[n] = select_classes(labels[s], C, seed, draw, n)
        take = selected[n][labels[s]] != 0
        out_i[n][take] = images[s][take]
        out_l[n][take] = labels[s][take]
    return out_i, out_l, selected


def validate(num_classes, labeler='self', thresholds=None, predict=None, mix=True, seed=0, teacher=None, has_average=False,
             model_thresholds=None, student=None):
    """The unlabelled-batch arguments of `FCN8s.train`; raises ValueError for what it refuses.  `labeler`: 'self', 'ema' or a model (anything
    with an `engine` that has `device` and `logical_classes`); `student`: the training model, for the comparison with such a labeler.
    Returns dict(labeler, thresholds float32[C], predict dict, mix, seed)."""
    Cn = int(num_classes)
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError("class mixing takes 2..{} classes, this model has {}".format(MAX_CLASSES, Cn))
    if teacher is not None:
        raise ValueError("`unlabeled_generator` together with `teacher`: the soft targets would have to cover the unlabelled rows of the "
                         "joined batch too; use one or the other.")
    if isinstance(labeler, str):
        if labeler not in ('self', 'ema'):
            raise ValueError("`unlabeled_labeler` must be 'self', 'ema' or another FCN8s, got {!r}".format(labeler))
        if labeler == 'ema' and not has_average:
            raise ValueError("unlabeled_labeler='ema' labels with the averaged weights: pass `ema_decay`, or train a model that holds an average.")
    else:
        eng = getattr(labeler, 'engine', None)
        if eng is None or not hasattr(eng, 'logical_classes'):
            raise ValueError("`unlabeled_labeler` must be 'self', 'ema' or another FCN8s, got {!r}".format(labeler))
        if student is not None:
            if labeler is student or eng is student.engine:
                raise ValueError("an `unlabeled_labeler` model must be another model (it is frozen for the call); 'self' labels with the student.")
            if eng.device != student.engine.device:
                raise ValueError("`unlabeled_labeler` must live on the student's device ({}), but is on {}.".format(student.engine.device, eng.device))
        if eng.logical_classes != Cn:
            raise ValueError("`unlabeled_labeler` has {} classes, the student {}.".format(eng.logical_classes, Cn))
    if thresholds is None:
        thresholds = model_thresholds
        if thresholds is None:
            raise ValueError("no thresholds: pass `unlabeled_thresholds` or run `fit_pseudo_label_thresholds` first.")
    if isinstance(thresholds, bool):
        raise ValueError("`unlabeled_thresholds` must be a number or one number per class")
    thr = np.asarray(thresholds, np.float32).reshape(-1)
    if thr.size == 1 and np.ndim(thresholds) == 0:
        thr = np.full(Cn, thr[0], np.float32)
    if thr.size != Cn:
        raise ValueError("`unlabeled_thresholds` must be a number or hold one value per class ({}), got {}".format(Cn, thr.size))
    if np.isnan(thr).any():
        raise ValueError("a threshold is NaN")
    kw = dict(predict or {})
    if set(kw) - set(PREDICT_KEYS):
        raise ValueError("`unlabeled_predict` takes `scales`, `flip`, `crf`, `temperature`, or `samples` / `keep_prob` / `mi_max`; got {}."
                         .format(sorted(kw)))
    if not isinstance(mix, (bool, np.bool_)):
        raise ValueError("`unlabeled_mix` must be True or False, got {!r}".format(mix))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 63:
        raise ValueError("`unlabeled_seed` must be an integer in [0, 2^63), got {!r}".format(seed))
    return dict(labeler=labeler, thresholds=np.ascontiguousarray(thr), predict=kw, mix=bool(mix), seed=int(seed))


# ---- the call on device tensors ------------------------------------------------------------------------------------------------------------
def work_bytes(N):
    from . import _lib as L
    return int(L.lib.fcn8s_op_class_mix_work_bytes(int(N)))


def flag_of(work, N):
    """The flag word of the most recent call on `work` for N images (1: a src[n] was out of range); synchronises."""
    import torch
    off = (-work.data_ptr()) % 16 + 288 * int(N)
    return int(work[off:off + 4].cpu().numpy().view(np.uint32)[0])


def mix_device(images, labels, src=None, seed=0, draw=0, num_classes=None, selected=False, work=None):
    """One `fcn8s_op_class_mix` call on uint8 device tensors [N,H,W,3] and [N,H,W], on the current stream: (images', labels', selected | None,
    work).  `src`: None = (n + 1) mod N, a sequence of N ints, or an int32 device tensor of N.  `work`: a uint8 device tensor to reuse (a larger
    one is made when it is too small) -- returned."""
    import ctypes as C
    import torch
    from . import _lib as L
    for t, rank, what in ((images, 4, "images"), (labels, 3, "labels")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != rank or not t.is_contiguous():
            raise ValueError("%s have to be a contiguous uint8 tensor of rank %d on the GPU" % (what, rank))
    if images.shape[-1] != 3 or tuple(images.shape[:3]) != tuple(labels.shape) or images.device != labels.device:
        raise ValueError("images [N,H,W,3] and labels [N,H,W] have to describe the same pixels on the same device")
    if num_classes is None:
        raise ValueError("class mixing needs the number of classes")
    _check_op(num_classes, seed, draw)
    N, H, W = (int(x) for x in labels.shape)
    dev = labels.device
    if src is None:
        src_t = (torch.arange(N, dtype=torch.int32, device=dev) + 1) % max(N, 1)
    elif isinstance(src, torch.Tensor):
        if src.dtype != torch.int32 or src.numel() != N or src.device != dev or not src.is_contiguous():
            raise ValueError("a src tensor is N contiguous int32 on the images' device")
        src_t = src
    else:
        a = np.asarray(src, np.int64).reshape(-1)
        if a.size != N or np.abs(a).max(initial=0) >= 1 << 31:
            raise ValueError("`src` holds one int32 per image")
        src_t = torch.from_numpy(a.astype(np.int32)).to(dev)
    nbytes = work_bytes(N)
    if work is None or work.numel() < nbytes or work.device != dev:
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out_i, out_l = torch.empty_like(images), torch.empty_like(labels)
    sel = torch.empty((N, 256), dtype=torch.uint8, device=dev) if selected else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.lib.fcn8s_op_class_mix(stream, C.c_void_p(images.data_ptr()), C.c_void_p(labels.data_ptr()), C.c_void_p(src_t.data_ptr()), N, H * W,
                                     int(num_classes), int(seed), int(draw), C.c_void_p(work.data_ptr()), C.c_void_p(out_i.data_ptr()),
                                     C.c_void_p(out_l.data_ptr()), C.c_void_p(sel.data_ptr()) if selected else None))
    return out_i, out_l, sel, work
