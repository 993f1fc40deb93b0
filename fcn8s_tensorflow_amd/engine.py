"""Thin Python owner of one `fcn8s_model` handle (one process, one GPU).

PyTorch-ROCm is plumbing here: it owns the flat parameter / gradient buffers
(so that `torch.distributed` = RCCL can all-reduce them and a torch optimizer
can update them) and provides the HIP stream.  All arithmetic of the FCN-8s
path happens inside libfcn8s_hip.so.

Data-parallel training: one Engine per rank, the minibatch is
sharded by the caller, gradients are all-reduced in four buckets in
backward-production order ({fc7, decoder} | {fc6} | {conv5, conv4} | {conv3..1});
a bucket's all-reduce starts behind the last kernel that writes into it
(fcn8s_bucket_wait) and runs on RCCL's stream while the rest of the backward
pass runs on the compute stream.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib as L
from . import crf as crf_mod
from . import loss as loss_mod
from . import optim as optim_mod
from . import tta
from . import mc_dropout
from .dp import BucketReducer


def _dist():
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


_CLASS_AXES = {   # axes of the decoder variables that run over classes (fcn8s_tensorflow.py:173-233)
    'pool3_1x1/kernel': (3,), 'pool3_1x1/bias': (0,), 'pool4_1x1/kernel': (3,), 'pool4_1x1/bias': (0,),
    'fc7_1x1/kernel': (3,), 'fc7_1x1/bias': (0,),
    'fc7_conv2d_trans/kernel': (2, 3), 'fc7_conv2d_trans/bias': (0,),
    'fc7_pool4_conv2d_trans/kernel': (2, 3), 'fc7_pool4_conv2d_trans/bias': (0,),
    'fc7_pool4_pool3_conv2d_trans/kernel': (2, 3), 'fc7_pool4_pool3_conv2d_trans/bias': (0,)}
_PAD_LOGIT = -1e30   # bias of a padding class in the last layer: its softmax probability is exactly 0, so is every gradient that touches it


def padded_classes(num_classes):
    """The library's class dimension: the next multiple of 4 (its C-channel tensors are accessed 16 bytes at a time)."""
    return (int(num_classes) + 3) // 4 * 4


def _pad_classes(name, a, c, cpad, slot=False):
    """Embed a decoder variable with `c` classes into the `cpad`-class shape: padding weights 0 (a padding channel then carries
    exactly 0 through the decoder and receives exactly 0 gradient -- the subspace is invariant under training), padding entries of
    the last bias _PAD_LOGIT."""
    axes = _CLASS_AXES.get(name)
    if axes is None or c == cpad:
        return a
    a = np.asarray(a)
    pad = [(0, cpad - c) if i in axes else (0, 0) for i in range(a.ndim)]
    fill = _PAD_LOGIT if (name == 'fc7_pool4_pool3_conv2d_trans/bias' and not slot) else 0.0
    return np.pad(a, pad, constant_values=fill)


def _unpad_classes(name, a, c, cpad):
    axes = _CLASS_AXES.get(name)
    if axes is None or c == cpad:
        return a
    sl = tuple(slice(0, c) if i in axes else slice(None) for i in range(np.ndim(a)))
    return np.ascontiguousarray(np.asarray(a)[sl])


class Staged:
    """One host batch on its way to the GPU through a staging slot (Engine.stage): pinned copy + H2D on the library's copy
    stream, started by whoever called stage() -- typically the feeder thread, while the compute stream runs the previous step."""
    __slots__ = ("slot", "img_ptr", "lab_ptr", "dtype", "nhw")

    def __init__(self, slot, img_ptr, lab_ptr, dtype, nhw):
        self.slot, self.img_ptr, self.lab_ptr, self.dtype, self.nhw = slot, img_ptr, lab_ptr, dtype, nhw


class Engine:
    def __init__(self, num_classes, widths=None, fc6_ksize=7, device_id=0, seed=0, process_group=None, precision='fp32', logical_classes=None,
                 options=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("fcn8s_tensorflow_amd needs an AMD GPU (gfx950); there is no CPU fallback for the hot path")
        self.torch = torch
        self.device = torch.device("cuda", device_id)
        torch.cuda.set_device(self.device)
        self.num_classes = int(num_classes)
        # classes the caller sees when `num_classes` was padded to the library's multiple of 4 (FCN8s facade): one-hot labels carry this many channels
        self.logical_classes = int(logical_classes) if logical_classes else int(num_classes)
        self.pg = process_group
        cfg = L.Config()
        cfg.num_classes = int(num_classes)
        cfg.fc6_ksize = int(fc6_ksize)
        for i in range(7):
            cfg.widths[i] = int(widths[i]) if widths else 0
        cfg.device_id = device_id
        cfg.seed = int(seed)
        n = L.lib.fcn8s_param_floats(C.byref(cfg))
        if n == 0:
            raise ValueError("invalid model configuration (num_classes must be a positive multiple of 4)")
        self.flat_params = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.flat_grads = torch.zeros(n, dtype=torch.float32, device=self.device)
        cfg.ext_params = self.flat_params.data_ptr()
        cfg.ext_grads = self.flat_grads.data_ptr()
        h = C.c_void_p()
        L.check(L.lib.fcn8s_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.widths = tuple(widths) if widths else (64, 128, 256, 512, 512, 4096, 4096)
        self.set_precision(precision)
        for k, v in (options or {}).items():        # algorithm variants for parity reports (include/fcn8s_hip.h: fcn8s_set_option)
            self.set_option(k, v)
        self.specs = OrderedDict()          # name -> (shape, offset)
        for i in range(L.lib.fcn8s_num_params(self.h)):
            name = C.c_char_p(); nd = C.c_int32(); shp = (C.c_int64 * 4)(); off = C.c_int64()
            L.check(L.lib.fcn8s_param_info(self.h, i, C.byref(name), C.byref(nd), C.byref(shp), C.byref(off)), self.h)
            self.specs[name.value.decode()] = (tuple(int(shp[k]) for k in range(nd.value)), int(off.value))
        self.buckets = []
        self.num_buckets = int(L.lib.fcn8s_num_buckets(self.h))
        self.native_comm = False                    # True: gradients are exchanged by the library's own RCCL communicator (comm_init_native)
        self._side = None
        for b in range(self.num_buckets):
            o = C.c_size_t(); m = C.c_size_t()
            L.check(L.lib.fcn8s_bucket_range(self.h, b, C.byref(o), C.byref(m)), self.h)
            self.buckets.append((o.value, m.value))
        self._label_checks_left = 2
        self._label_calls = 0
        self._bad = None
        self.loss_config = None              # set_loss: the training loss's configuration (None = the reference's mean)
        self.lovasz_config = None            # set_lovasz: the Lovász-softmax term's configuration (None = off)
        self.boundary_config = None          # set_boundary_loss: the boundary weighting's configuration, dict(table, radius) (None = off)
        self.soft_target_config = None       # set_soft_targets: the soft-target term's configuration, dict(weight, temperature, pixels) (None = off)
        self._soft_targets = None            # bind_soft_targets: the bound tensor, kept alive until a training loss has consumed it
        self.entropy_config = None           # set_entropy_term: the entropy term's configuration, dict(weight, pixels, first_image) (None = off)
        self.focal_config = None             # set_focal: the focal loss's configuration, dict(gamma) (None = off)
        self._loss_shape = None              # (N, H, W) of the last training loss (boundary_codes)
        self.grad_clip = None                # set_grad_clip: the global-norm clip's max_norm (None = off; inf = the non-finite guard alone)
        self.ema_config = None               # set_ema: the parameter average's configuration, dict(decay, warmup) (None = off)
        self.replica_check_every = 100      # data-parallel runs: compare global step + parameter checksum across ranks every so many steps (0 = never)
        self._sync_stream()

    # ---- plumbing ---------------------------------------------------------------------
    def _sync_stream(self):
        L.check(L.lib.fcn8s_set_stream(self.h, C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)), self.h)

    def close(self):
        if getattr(self, "h", None) is not None:
            self.torch.cuda.synchronize(self.device)
            L.lib.fcn8s_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def world_size(self):
        if getattr(self, "native_comm", False):
            return self.comm_world
        d = _dist()
        return d.get_world_size(self.pg) if d else 1

    @property
    def rank(self):
        if getattr(self, "native_comm", False):
            return self.comm_rank
        d = _dist()
        return d.get_rank(self.pg) if d else 0

    # ---- variables -----------------------------------------------------------------------
    def param_view(self, name):
        shape, off = self.specs[name]
        return self.flat_params[off:off + int(np.prod(shape))].view(*shape)

    def logical_param_view(self, name):
        """param_view without the padding classes (a strided view when num_classes was padded to a multiple of 4)."""
        v = self.param_view(name)
        if self.logical_classes != self.num_classes:
            for ax in _CLASS_AXES.get(name, ()):
                v = v.narrow(ax, 0, self.logical_classes)
        return v

    def grad_view(self, name):
        shape, off = self.specs[name]
        return self.flat_grads[off:off + int(np.prod(shape))].view(*shape)

    def set_params(self, params):
        for k, v in params.items():
            if k not in self.specs:
                raise ValueError("unknown variable '%s'" % k)
            a = np.ascontiguousarray(self.pad(k, np.asarray(v, dtype=np.float32)), dtype=np.float32)
            if tuple(a.shape) != self.specs[k][0]:
                raise ValueError("variable '%s' has shape %s, expected %s" % (k, a.shape, self.specs[k][0]))
            L.check(L.lib.fcn8s_set_param(self.h, k.encode(), a.ctypes.data_as(C.c_void_p), a.size), self.h)

    def get_params(self):
        out = OrderedDict()
        for k, (shape, _) in self.specs.items():
            a = np.empty(shape, np.float32)
            L.check(L.lib.fcn8s_get_param(self.h, k.encode(), a.ctypes.data_as(C.c_void_p), a.size), self.h)
            out[k] = self.unpad(k, a)
        return out

    def get_grads(self):
        out = OrderedDict()
        for k, (shape, _) in self.specs.items():
            a = np.empty(shape, np.float32)
            L.check(L.lib.fcn8s_get_grad(self.h, k.encode(), a.ctypes.data_as(C.c_void_p), a.size), self.h)
            out[k] = self.unpad(k, a)
        return out

    def pad(self, name, a, slot=False):
        """A variable (or, slot=True, one of its optimizer slots) with `logical_classes` classes in the library's padded shape."""
        return _pad_classes(name, a, self.logical_classes, self.num_classes, slot)

    def unpad(self, name, a):
        return _unpad_classes(name, a, self.logical_classes, self.num_classes)

    def init_params(self, seed=0):
        self._sync_stream()
        L.check(L.lib.fcn8s_init_params(self.h, int(seed)), self.h)
        if self.logical_classes != self.num_classes:           # padding classes: zero weights, probability-0 bias in the last layer
            c = self.logical_classes
            for name, axes in _CLASS_AXES.items():
                v = self.param_view(name)
                fill = _PAD_LOGIT if name == 'fc7_pool4_pool3_conv2d_trans/bias' else 0.0
                for ax in axes:
                    v.narrow(ax, c, self.num_classes - c).fill_(fill)

    def broadcast_params(self, src=0):
        if self.native_comm:
            self._sync_stream()
            L.check(L.lib.fcn8s_comm_broadcast_params(self.h, int(src)), self.h)
            return
        d = _dist()
        if d and self.world_size > 1:
            self.freeze(False)
            d.broadcast(self.flat_params, src=src, group=self.pg)

    @property
    def global_step(self):
        return int(L.lib.fcn8s_global_step(self.h))

    @global_step.setter
    def global_step(self, v):
        L.check(L.lib.fcn8s_set_global_step(self.h, int(v)), self.h)

    def get_opt_state(self):
        n = self.flat_params.numel()
        m = np.empty(n, np.float32); v = np.empty(n, np.float32)
        L.check(L.lib.fcn8s_get_opt_state(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), n), self.h)
        return m, v

    def set_opt_state(self, m, v):
        m = np.ascontiguousarray(m, np.float32); v = np.ascontiguousarray(v, np.float32)
        L.check(L.lib.fcn8s_set_opt_state(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), m.size), self.h)

    # ---- input marshalling -----------------------------------------------------------------
    def _images(self, images, force_device=False):
        """-> (keepalive, pointer, dtype code, where, (N,H,W))"""
        torch = self.torch
        if isinstance(images, (list, tuple)):
            images = np.asarray(images)
        if isinstance(images, torch.Tensor):
            t = images
            if t.dim() != 4 or t.shape[-1] != 3:
                raise ValueError("images must have shape (batch, height, width, 3)")
            if t.dtype not in (torch.uint8, torch.float32):
                t = t.float()
            if t.is_cuda or force_device:
                t = t.to(self.device).contiguous()
                return t, C.c_void_p(t.data_ptr()), (L.IMG_U8 if t.dtype == torch.uint8 else L.IMG_F32), L.DEVICE, tuple(t.shape[:3])
            images = t.numpy()
        a = np.asarray(images)
        if a.ndim != 4 or a.shape[-1] != 3:
            raise ValueError("images must be an array-like of rank 4 with shape (batch, height, width, 3)")
        if a.dtype != np.uint8:
            a = a.astype(np.float32, copy=False)
        a = np.ascontiguousarray(a)
        if force_device:
            t = torch.from_numpy(a).to(self.device)
            return t, C.c_void_p(t.data_ptr()), (L.IMG_U8 if a.dtype == np.uint8 else L.IMG_F32), L.DEVICE, a.shape[:3]
        return a, a.ctypes.data_as(C.c_void_p), (L.IMG_U8 if a.dtype == np.uint8 else L.IMG_F32), L.HOST, a.shape[:3]

    def _check_ids(self, ids):
        """Class ids that would select a padding class (num_classes padded to a multiple of 4 by the facade) are an error, as
        `np.eye(num_classes)[ids]` is in the reference (helpers/ground_truth_conversion_utils.py:84-88: IndexError); ids at or above
        the padded count stay what include/fcn8s_hip.h says they are: 'ignore'.  Only costs anything when classes are padded."""
        if self.logical_classes == self.num_classes:
            return
        lo, hi = self.logical_classes, self.num_classes
        if isinstance(ids, np.ndarray):
            bad = bool(((ids >= lo) & (ids < hi)).any())
        else:
            bad = bool(((ids >= lo) & (ids < hi)).any().item())
        if bad:
            raise ValueError("class ids must be below num_classes = %d (ids from %d on mean 'ignore')" % (lo, hi))

    def _onehot_to_ids(self, t, nhw):
        """One-hot rows (N,H,W,C) on the device -> uint8 class ids on the device (library kernel).
        The first batches are also checked for being one-hot (costs one host sync each)."""
        torch = self.torch
        if t.shape[-1] != self.logical_classes:
            raise ValueError("one-hot labels must have %d channels, got %d" % (self.logical_classes, t.shape[-1]))
        if tuple(t.shape[:3]) != tuple(nhw):
            raise ValueError("labels shape %s does not match images %s" % (tuple(t.shape), tuple(nhw)))
        if t.dtype in (torch.bool, torch.uint8, torch.int8):
            eb = 1
        elif t.dtype in (torch.int32, torch.float32):
            eb = 4
        else:
            t = t.to(torch.int32); eb = 4
        t = t.to(self.device).contiguous()
        npix = int(nhw[0]) * int(nhw[1]) * int(nhw[2])
        ids = torch.empty(tuple(int(x) for x in nhw), dtype=torch.uint8, device=self.device)
        # every batch adds its count of rows that are not one-hot to a device counter (no sync); the host looks at it on the first
        # two batches and then every 64th (all-zero rows train as "ignore", multi-hot rows as their first class -- see include/fcn8s_hip.h)
        if self._bad is None:
            self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib.fcn8s_onehot_to_ids(stream, C.c_void_p(t.data_ptr()), eb, npix, self.logical_classes,
                                          C.c_void_p(ids.data_ptr()), C.c_void_p(self._bad.data_ptr())))
        self._label_calls += 1
        if self._label_checks_left > 0 or self._label_calls % 64 == 0:
            self._label_checks_left = max(0, self._label_checks_left - 1)
            nbad = int(self._bad.item())
            if nbad:
                self._bad.zero_()
                raise ValueError("labels must be one-hot along the last axis (%d rows of the last %s were not); "
                                 "soft targets go through set_soft_targets / bind_soft_targets, not through the labels" % (nbad, "batch" if self._label_calls <= 2 else "64 batches"))
        return ids

    def _inputs(self, images, labels):
        """Marshals one (images, labels) feed.  One-hot labels (the reference's format, fcn8s_tensorflow.py:110,
        429-433) are shipped to the GPU and reduced to uint8 class ids there -- an np.argmax over the
        168 MB one-hot batch on the host would cost more than the whole training step."""
        torch = self.torch
        if isinstance(images, Staged):
            st = images
            L.check(L.lib.fcn8s_stage_wait(self.h, st.slot), self.h)
            return st, C.c_void_p(st.img_ptr), st.dtype, C.c_void_p(st.lab_ptr) if st.lab_ptr else None, L.DEVICE, st.nhw
        lab_is_tensor = isinstance(labels, torch.Tensor)
        lab_rank = labels.dim() if lab_is_tensor else np.ndim(labels)
        onehot = lab_rank == 4
        ka_i, pi, dt, where, nhw = self._images(images, force_device=onehot or (lab_is_tensor and labels.is_cuda))
        if onehot:
            t = labels if lab_is_tensor else torch.from_numpy(np.ascontiguousarray(labels))
            ids = self._onehot_to_ids(t, nhw)
            return (ka_i, ids), pi, dt, C.c_void_p(ids.data_ptr()), where, nhw
        if lab_rank != 3:
            raise ValueError("labels must be one-hot (batch, height, width, num_classes) or class ids (batch, height, width)")
        if lab_is_tensor:
            t = labels
            if tuple(t.shape) != tuple(nhw):
                raise ValueError("labels shape %s does not match images %s" % (tuple(t.shape), tuple(nhw)))
            t = t.to(torch.uint8).contiguous()
            if where == L.DEVICE:
                t = t.to(self.device)
                self._check_ids(t)
                return (ka_i, t), pi, dt, C.c_void_p(t.data_ptr()), where, nhw
            labels = t.cpu().numpy()
        a = np.asarray(labels)
        if tuple(a.shape) != tuple(nhw):
            raise ValueError("labels shape %s does not match images %s" % (tuple(a.shape), tuple(nhw)))
        a = np.ascontiguousarray(a, dtype=np.uint8)
        self._check_ids(a)
        if where == L.DEVICE:
            t = torch.from_numpy(a).to(self.device)
            return (ka_i, t), pi, dt, C.c_void_p(t.data_ptr()), where, nhw
        return (ka_i, a), pi, dt, a.ctypes.data_as(C.c_void_p), where, nhw

    def stage(self, images, label_ids=None, slot=0):
        """Start moving one host batch to the GPU (include/fcn8s_hip.h: fcn8s_stage_inputs) and return a `Staged` handle that
        train_step / eval_step / predict accept in place of the arrays.  images: uint8 or float32 array (N,H,W,3); label_ids:
        uint8 class ids (N,H,W) or None.  Thread-safe against the compute calls of this engine (it only touches the staging slot
        and the copy stream), so a feeder thread can stage batch k+1 while step k runs."""
        a = np.asarray(images)
        if a.ndim != 4 or a.shape[-1] != 3:
            raise ValueError("images must be an array-like of rank 4 with shape (batch, height, width, 3)")
        if a.dtype != np.uint8:
            a = a.astype(np.float32, copy=False)
        a = np.ascontiguousarray(a)
        lab = None
        if label_ids is not None:
            lab = np.ascontiguousarray(label_ids, dtype=np.uint8)
            if tuple(lab.shape) != tuple(a.shape[:3]):
                raise ValueError("labels shape %s does not match images %s" % (tuple(lab.shape), tuple(a.shape[:3])))
            self._check_ids(lab)
        pi, pl = C.c_void_p(), C.c_void_p()
        N, H, W = (int(x) for x in a.shape[:3])
        dt = L.IMG_U8 if a.dtype == np.uint8 else L.IMG_F32
        L.check(L.lib.fcn8s_stage_inputs(self.h, int(slot), a.ctypes.data_as(C.c_void_p), dt,
                                         lab.ctypes.data_as(C.c_void_p) if lab is not None else None, N, H, W, C.byref(pi), C.byref(pl)), self.h)
        return Staged(int(slot), pi.value, pl.value, dt, (N, H, W))

    def _release(self, ka):
        if isinstance(ka, Staged):
            L.check(L.lib.fcn8s_stage_release(self.h, ka.slot), self.h)

    # ---- hot path ----------------------------------------------------------------------------
    def freeze(self, frozen=True):
        """Promise (or withdraw the promise) that the parameters stay constant: inside evaluate() / predict loops the library then
        keeps the Winograd-transformed filter banks across calls.  Library calls that change parameters unfreeze on their own;
        code that writes into `flat_params` through torch must call `freeze(False)` first."""
        L.check(L.lib.fcn8s_freeze_params(self.h, 1 if frozen else 0), self.h)

    def set_option(self, key, value):
        """fcn8s_set_option: 'winograd_min_cin', 'winograd_tile', 'winograd_fc6', 'fc6_fft', 'fc6_fft_wgrad', 'tconv_gemm' (defaults = the measured winners)."""
        L.check(L.lib.fcn8s_set_option(self.h, key.encode(), int(value)), self.h)

    def get_option(self, key):
        v = C.c_int64()
        L.check(L.lib.fcn8s_get_option(self.h, key.encode(), C.byref(v)), self.h)
        return int(v.value)

    def set_precision(self, precision):
        """'fp32' (the reference's arithmetic), 'bf16_fc' (BASELINE config 5: forward fc6 / fc7 with bf16-rounded
        operands on the bf16 MFMA, fp32 accumulation; the rest of the step stays fp32), 'f32x3' (every large GEMM on the
        bf16 MFMA with each fp32 operand split exactly into three bf16 pieces: fp32 accuracy, not bit-identical to fp32) or
        'bf16_fwd' (config 5 taken further: conv3_1 .. conv5_3, fc6 and fc7 forward with bf16-rounded operands, every other GEMM
        in the f32x3 arithmetic: all matrix work on the bf16 MFMA); 'f32x2' / 'bf16_fwd_x2' = 'f32x3' / 'bf16_fwd' with two bf16
        pieces per operand instead of three (16 significand bits enter each product: reduced precision, half the matrix work);
        'bf16_train' = mixed-precision training as it is usually meant: conv1_2 .. conv5_3, fc6 and fc7 as direct convolutions whose operands are
        rounded to bf16 in the forward pass, the data gradient AND the weight gradient (fp32 accumulate, fp32 master weights, everything else
        exact fp32; no Winograd transforms); 'fp8_infer' = inference only: conv1_2 .. conv5_3, fc6 and fc7 with OCP e4m3 operands on the
        block-scaled MX MFMA, static per-layer activation scales from `calibrate_fp8` and per-channel weight scales (fp8.py states the
        arithmetic); training calls refuse it."""
        modes = {'fp32': L.PREC_F32, 'bf16_fc': L.PREC_BF16_FC, 'f32x3': L.PREC_F32X3, 'bf16_fwd': L.PREC_BF16_FWD,
                 'f32x2': L.PREC_F32X2, 'bf16_fwd_x2': L.PREC_BF16_FWD_X2, 'bf16_train': L.PREC_BF16_TRAIN, 'fp8_infer': L.PREC_FP8_INFER}
        if precision not in modes:
            raise ValueError("`precision` must be 'fp32', 'bf16_fc', 'f32x3', 'bf16_fwd', 'f32x2', 'bf16_fwd_x2', 'bf16_train' or 'fp8_infer', "
                             "but is '{}'.".format(precision))
        L.check(L.lib.fcn8s_set_precision(self.h, modes[precision]), self.h)
        self.precision = precision

    def set_loss(self, class_weights=None, ohem_thresh=None, ohem_min_kept=100000):
        """The training loss (fcn8s_set_loss; definitions in loss.py and include/fcn8s_hip.h): per-class weights in the caller's logical
        class count (padded here with zeros to the library's multiple of 4) and / or OHEM with a probability threshold in (0, 1] and at
        least `ohem_min_kept` pixels kept.  No arguments restore the reference's mean.  Evaluation keeps the reference's loss."""
        w, t, k = loss_mod.validate(class_weights, ohem_thresh, ohem_min_kept, self.logical_classes)
        if w is not None:
            w = np.concatenate([w, np.zeros(self.num_classes - w.size, np.float32)]).astype(np.float32)
            arr = (C.c_float * w.size)(*w.tolist())
            L.check(L.lib.fcn8s_set_loss(self.h, arr, int(w.size), t, k), self.h)
        else:
            L.check(L.lib.fcn8s_set_loss(self.h, None, 0, t, k), self.h)
        self.loss_config = None if (w is None and t == 0.0) else dict(
            class_weights=None if class_weights is None else np.asarray(class_weights, np.float32).copy(),
            ohem_thresh=ohem_thresh if t else None, ohem_min_kept=k)

    def set_lovasz(self, lovasz_weight, ce_weight=1.0, per_image=False, classes='present'):
        """The Lovász-softmax term of the training loss (fcn8s_set_lovasz; definitions in include/fcn8s_hip.h, restated in loss.py):
        L = ce_weight * (the cross-entropy of set_loss) + lovasz_weight * L_lov + L2.  `per_image` sorts each image on its own;
        `classes` is 'present', 'all' or a list of logical class ids (the padding classes never take part).  set_lovasz(0) restores the
        default.  Evaluation keeps the reference's loss."""
        ce, lov, pi, ca, mask = loss_mod.validate_lovasz(lovasz_weight, ce_weight, per_image, classes, self.logical_classes)
        full = np.zeros(self.num_classes, np.uint8)
        full[:self.logical_classes] = mask
        arr = (C.c_uint8 * self.num_classes)(*full.tolist())
        L.check(L.lib.fcn8s_set_lovasz(self.h, ce, lov, pi, ca, arr, self.num_classes), self.h)
        self.lovasz_config = None if (lov == 0.0 and ce == 1.0) else dict(
            lovasz_weight=lov, ce_weight=ce, per_image=bool(pi), classes=classes if isinstance(classes, str) else list(classes))

    def set_boundary_loss(self, table=None, radius=None):
        """The boundary weighting of the training cross-entropy (fcn8s_set_boundary_loss; definitions in include/fcn8s_hip.h, restated in
        loss.py): every training loss computes the distance codes of its own labels and weights pixel p by w_{y_p} * table[code(p)].
        `table` = 256 weights per distance code (loss.boundary_table, loss.ignore_band_table, loss.resolve_boundary), `radius` in 1..15.
        No arguments restore the default.  Evaluation keeps the reference's loss."""
        T, R = loss_mod.validate_boundary(table, radius)
        if T is None:
            L.check(L.lib.fcn8s_set_boundary_loss(self.h, 0, None), self.h)
        else:
            arr = (C.c_float * 256)(*T.tolist())
            L.check(L.lib.fcn8s_set_boundary_loss(self.h, R, arr), self.h)
        self.boundary_config = None if T is None else dict(table=T.copy(), radius=R)

    def boundary_codes(self):
        """The uint8 [N, H, W] distance codes the last training loss computed from its labels (fcn8s_get_boundary_codes; synchronises)."""
        out = np.empty(self._loss_shape or (1, 1, 1), np.uint8)      # (before any training loss the library answers with its state error)
        L.check(L.lib.fcn8s_get_boundary_codes(self.h, out.ctypes.data_as(C.c_void_p), int(out.size)), self.h)
        return out

    def loss_terms(self):
        """The unscaled terms of the last training loss: dict(ce, lovasz, l2) (fcn8s_get_loss_terms; synchronises)."""
        ce = C.c_float(); lv = C.c_float(); l2 = C.c_float()
        L.check(L.lib.fcn8s_get_loss_terms(self.h, C.byref(ce), C.byref(lv), C.byref(l2)), self.h)
        return dict(ce=float(ce.value), lovasz=float(lv.value), l2=float(l2.value))

    def set_soft_targets(self, weight=None, temperature=1.0, pixels='valid'):
        """The soft-target (distillation) term of the training loss (fcn8s_set_soft_targets; definitions in include/fcn8s_hip.h, restated in
        loss.py): L += weight * L_kd, L_kd = (T^2 / P) sum_p KL(teacher_p || student_p) at `temperature` over the pixels with a valid label
        (`pixels` = 'valid') or over every pixel ('all': a batch whose labels are all "ignore" still has a loss).  Every training loss then
        needs targets bound with bind_soft_targets first.  No weight (or 0) switches the term off and drops a binding.  Evaluation and
        prediction keep the reference's loss."""
        w, t, ap = loss_mod.validate_soft_targets(weight, temperature, pixels)
        L.check(L.lib.fcn8s_set_soft_targets(self.h, w, t, ap), self.h)
        if w == 0.0:
            self._soft_targets = None
        self.soft_target_config = None if w == 0.0 else dict(weight=w, temperature=t, pixels=pixels)

    def bind_soft_targets(self, probs):
        """The targets of the NEXT training loss (fcn8s_bind_soft_targets): a cuda float32 tensor [N, H, W, logical_classes] whose last
        dimension has unit stride and whose rows are evenly spaced -- a contiguous tensor, or the view predict(argmax=False) returns under
        padded classes, which is bound through its row stride without a copy.  The tensor is kept alive until a training loss has consumed
        it; the loss reads it on the engine's stream (torch's current one), so a tensor produced on that stream needs no further ordering."""
        torch = self.torch
        if not isinstance(probs, torch.Tensor) or probs.device != self.device or probs.dtype != torch.float32:
            raise ValueError("soft targets must be a float32 tensor on %s" % (self.device,))
        if probs.dim() != 4 or probs.shape[-1] != self.logical_classes:
            raise ValueError("soft targets must be [N, H, W, %d], got %s" % (self.logical_classes, tuple(probs.shape)))
        N, H, W, K = (int(x) for x in probs.shape)
        sn, sh, sw, sc = (int(x) for x in probs.stride())
        if (K > 1 and sc != 1) or sw < K or (W > 1 and sh != W * sw) or (H > 1 and sn != H * W * sw):
            raise ValueError("soft targets need a unit last-dimension stride and evenly spaced rows (strides %s): pass a contiguous tensor "
                             "or a class-slice of one" % ((sn, sh, sw, sc),))
        L.check(L.lib.fcn8s_bind_soft_targets(self.h, C.c_void_p(probs.data_ptr()), N, H, W, K, sw), self.h)
        self._soft_targets = probs

    def soft_target_term(self):
        """The unscaled L_kd of the last training loss (fcn8s_get_soft_target_term; synchronises); raises if that loss ran without the term."""
        kd = C.c_float()
        L.check(L.lib.fcn8s_get_soft_target_term(self.h, C.byref(kd)), self.h)
        return float(kd.value)

    def set_entropy_term(self, weight=None, pixels='unlabeled', first_image=0):
        """The entropy term of the training loss (fcn8s_set_entropy_term; definitions in include/fcn8s_hip.h, restated in loss.py):
        L += weight * L_ent, L_ent = (1 / (P log K)) sum_{p in U} h_p, h_p the entropy of the student's own softmax over the K =
        `logical_classes` classes; U = the pixels of the images >= `first_image` that have no label (`pixels` = 'unlabeled': id >= num_classes),
        a label ('valid') or either ('all').  A positive weight minimises the entropy (Grandvalet & Bengio 2005; ADVENT's MinEnt), a negative
        one is the confidence penalty (Pereyra et al. 2017).  No weight (or 0) switches the term off.  Host state only: nothing is launched,
        allocated or waited for.  Evaluation and prediction keep the reference's loss."""
        w, ps, first = loss_mod.validate_entropy_term(weight, pixels, first_image)
        if w != 0.0 and self.logical_classes < 2:
            raise ValueError("the entropy term needs at least 2 classes, the model has %d" % self.logical_classes)
        L.check(L.lib.fcn8s_set_entropy_term(self.h, w, ps, self.logical_classes if w != 0.0 else self.num_classes, first), self.h)
        self.entropy_config = None if w == 0.0 else dict(weight=w, pixels=pixels, first_image=first)

    def entropy_term(self):
        """The unscaled L_ent of the last training loss (fcn8s_get_entropy_term; synchronises); raises if that loss ran without the term."""
        v = C.c_float()
        L.check(L.lib.fcn8s_get_entropy_term(self.h, C.byref(v)), self.h)
        return float(v.value)

    def entropy_term_op(self, logits, labels, weight=1.0, pixels='unlabeled', ncols=None, first_image=0, dlogits=None, bias=False):
        """One `fcn8s_op_entropy_term` call on device tensors, on the current stream: `logits` float32 [N, ..., C] (contiguous), `labels` uint8
        [N, ...] of the same pixels.  `dlogits` (a float32 tensor of the logits' shape, or None) gets the gradient contribution added in
        place.  Returns (term, bias | None): device tensors of 1 and (with `bias`) C floats; nothing synchronises.  The scratch is kept on the
        engine."""
        torch = self.torch
        w, ps, first = loss_mod.validate_entropy_term(weight, pixels, first_image)
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() < 2 or not logits.is_contiguous():
            raise ValueError("logits have to be a contiguous float32 tensor [N, ..., C] on the GPU")
        if not isinstance(labels, torch.Tensor) or labels.device != logits.device or labels.dtype != torch.uint8 or not labels.is_contiguous() \
                or tuple(labels.shape) != tuple(logits.shape[:-1]):
            raise ValueError("labels have to be a contiguous uint8 tensor of the logits' pixels on the same device")
        if dlogits is not None and (not isinstance(dlogits, torch.Tensor) or dlogits.device != logits.device or dlogits.dtype != torch.float32
                                    or tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous()):
            raise ValueError("dlogits have to be a contiguous float32 tensor of the logits' shape on the same device")
        N, Cn = int(logits.shape[0]), int(logits.shape[-1])
        HW = int(labels.numel()) // max(N, 1)
        nbytes = int(L.lib.fcn8s_op_entropy_term_work_bytes())
        work = getattr(self, "_entropy_work", None)
        if work is None or work.numel() < nbytes or work.device != logits.device:
            work = self._entropy_work = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
        term = torch.empty(1, dtype=torch.float32, device=logits.device)
        b = torch.empty(Cn, dtype=torch.float32, device=logits.device) if bias else None
        stream = C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
        L.check(L.lib.fcn8s_op_entropy_term(stream, C.c_void_p(logits.data_ptr()), C.c_void_p(dlogits.data_ptr()) if dlogits is not None else None,
                                            C.c_void_p(labels.data_ptr()), N, HW, Cn, Cn if ncols is None else int(ncols), ps, first, w,
                                            C.c_void_p(work.data_ptr()), nbytes, C.c_void_p(term.data_ptr()),
                                            C.c_void_p(b.data_ptr()) if bias else None))
        return term, b

    def set_focal(self, gamma=None):
        """The focal loss of training (fcn8s_set_focal; definitions in include/fcn8s_hip.h, restated in loss.py): the per-pixel cross-entropy
        l_p becomes (1 - p_y)^gamma l_p, `gamma` in (0, 8] (2 is the paper's default).  The class weights of set_loss act as its alpha, the
        boundary table acts on it, the Lovász, soft-target and entropy terms add behind it; OHEM and the focal loss refuse each other.  No gamma
        (or 0) switches it off.  Host state only: nothing is launched, allocated or waited for.  Evaluation and prediction keep the reference's
        loss."""
        g = loss_mod.validate_focal(gamma, (self.loss_config or {}).get('ohem_thresh'))
        L.check(L.lib.fcn8s_set_focal(self.h, g), self.h)
        self.focal_config = None if g == 0.0 else dict(gamma=g)

    def focal_xent_op(self, logits, labels, gamma, class_weights=None, codes=None, table=None, dlogits=None, bias=False):
        """One `fcn8s_op_focal_xent` call on device tensors, on the current stream: `logits` float32 [N, ..., C] (contiguous), `labels` uint8
        [N, ...] of the same pixels, `class_weights` a float32 device tensor of C weights or None, `codes` (uint8, the labels' shape) and `table`
        (256 float32) both given or both None.  `dlogits` (a float32 tensor of the logits' shape, or None) is overwritten by the gradient.
        Returns (loss, bias | None): device tensors of 1 and (with `bias`) C floats; nothing synchronises.  The scratch is kept on the engine."""
        torch = self.torch
        g = loss_mod.validate_focal(gamma)
        if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() < 2 or not logits.is_contiguous():
            raise ValueError("logits have to be a contiguous float32 tensor [N, ..., C] on the GPU")
        if not isinstance(labels, torch.Tensor) or labels.device != logits.device or labels.dtype != torch.uint8 or not labels.is_contiguous() \
                or tuple(labels.shape) != tuple(logits.shape[:-1]):
            raise ValueError("labels have to be a contiguous uint8 tensor of the logits' pixels on the same device")
        if dlogits is not None and (not isinstance(dlogits, torch.Tensor) or dlogits.device != logits.device or dlogits.dtype != torch.float32
                                    or tuple(dlogits.shape) != tuple(logits.shape) or not dlogits.is_contiguous()):
            raise ValueError("dlogits have to be a contiguous float32 tensor of the logits' shape on the same device")
        Cn = int(logits.shape[-1])
        if class_weights is not None and (not isinstance(class_weights, torch.Tensor) or class_weights.device != logits.device
                                          or class_weights.dtype != torch.float32 or class_weights.numel() != Cn or not class_weights.is_contiguous()):
            raise ValueError("class_weights have to be a contiguous float32 tensor of C = %d weights on the same device" % Cn)
        if (codes is None) != (table is None):
            raise ValueError("codes and table have to be given together")
        if codes is not None:
            if not isinstance(codes, torch.Tensor) or codes.device != logits.device or codes.dtype != torch.uint8 or not codes.is_contiguous() \
                    or tuple(codes.shape) != tuple(labels.shape):
                raise ValueError("codes have to be a contiguous uint8 tensor of the labels' shape on the same device")
            if not isinstance(table, torch.Tensor) or table.device != logits.device or table.dtype != torch.float32 or table.numel() != 256 \
                    or not table.is_contiguous():
                raise ValueError("table has to be a contiguous float32 tensor of 256 weights on the same device")
        nbytes = int(L.lib.fcn8s_op_focal_xent_work_bytes())
        work = getattr(self, "_focal_work", None)
        if work is None or work.numel() < nbytes or work.device != logits.device:
            work = self._focal_work = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        b = torch.empty(Cn, dtype=torch.float32, device=logits.device) if bias else None
        stream = C.c_void_p(torch.cuda.current_stream(logits.device).cuda_stream)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        L.check(L.lib.fcn8s_op_focal_xent(stream, ptr(logits), ptr(labels), ptr(class_weights), ptr(codes), ptr(table), g, ptr(dlogits), ptr(loss), ptr(b),
                                          int(labels.numel()), Cn, ptr(work), nbytes))
        return loss, b

    def loss_stats(self):
        """|V|, |K| and the threshold t of the last training loss (fcn8s_get_loss_stats; synchronises)."""
        v = C.c_int64(); kp = C.c_int64(); t = C.c_float()
        L.check(L.lib.fcn8s_get_loss_stats(self.h, C.byref(v), C.byref(kp), C.byref(t)), self.h)
        return dict(valid=int(v.value), kept=int(kp.value), threshold=float(t.value))

    def set_grad_clip(self, max_norm):
        """The update's global-norm clip (fcn8s_set_grad_clip; definitions in include/fcn8s_hip.h, restated in optim.py): every update
        first takes the norm of the (all-reduced, scaled) gradient on the device and multiplies the gradient by
        max_norm / max(norm, max_norm) inside the optimizer kernel; an update whose norm is not finite is skipped.  `max_norm` in
        (0, inf] -- inf = the guard alone --, None or 0 = off.  No host round trip: read the numbers with update_stats()."""
        v = optim_mod.validate_clip(max_norm)
        L.check(L.lib.fcn8s_set_grad_clip(self.h, v), self.h)
        self.grad_clip = v if v > 0 else None

    def update_stats(self):
        """norm, clip_coef and scale of the last update and the updates skipped so far (fcn8s_get_update_stats; synchronises)."""
        n = C.c_float(); c = C.c_float(); sc = C.c_float(); k = C.c_int64()
        L.check(L.lib.fcn8s_get_update_stats(self.h, C.byref(n), C.byref(c), C.byref(sc), C.byref(k)), self.h)
        return dict(norm=float(n.value), clip_coef=float(c.value), scale=float(sc.value), skipped=int(k.value))

    # ---- the average of the parameters (fcn8s_set_ema; definitions in include/fcn8s_hip.h, restated in optim.py) -------------------
    def set_ema(self, decay, warmup=True):
        """Keep an exponential moving average of the parameters on the device: after every applied update
        s <- s - (1 - d_t) (s - theta), d_t = min(decay, (1 + t) / (10 + t)) with `warmup` (TensorFlow's num_updates rule), else decay.
        The shadow is allocated, and set to the parameters, when the average is first switched on; `decay` None or 0 switches it off and
        keeps the shadow.  The update folds the new parameters into the shadow in its own pass; a skipped update leaves it alone."""
        d, w = optim_mod.validate_ema(decay, warmup)
        self._sync_stream()
        L.check(L.lib.fcn8s_set_ema(self.h, d, int(w)), self.h)
        self.ema_config = dict(decay=d, warmup=w) if d > 0 else None

    def ema_info(self):
        """dict(decay, warmup, has_shadow, swapped) as the library holds them (fcn8s_get_ema_info)."""
        d = C.c_double(); w = C.c_int(); hs = C.c_int(); sw = C.c_int()
        L.check(L.lib.fcn8s_get_ema_info(self.h, C.byref(d), C.byref(w), C.byref(hs), C.byref(sw)), self.h)
        return dict(decay=float(d.value), warmup=bool(w.value), has_shadow=bool(hs.value), swapped=bool(sw.value))

    def ema_reset(self):
        """shadow = parameters (a device copy on the stream)."""
        self._sync_stream()
        L.check(L.lib.fcn8s_ema_reset(self.h), self.h)

    def get_ema(self):
        """The flat shadow in the library's padded layout, like get_opt_state's arrays.  While swapped it holds the raw weights."""
        a = np.empty(self.flat_params.numel(), np.float32)
        L.check(L.lib.fcn8s_get_ema(self.h, a.ctypes.data_as(C.c_void_p), a.size), self.h)
        return a

    def set_ema_state(self, a):
        """Write the flat shadow (allocating it if there is none); does not switch the average on."""
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        L.check(L.lib.fcn8s_set_ema_state(self.h, a.ctypes.data_as(C.c_void_p), a.size), self.h)

    def ema_swap(self):
        """Exchange the parameters and the shadow in place (one kernel).  While swapped every consumer of the parameters -- evaluation,
        prediction, fp8 calibration, get_params, save -- sees the averaged weights and every training call raises; a second swap restores
        the raw weights bit for bit.  Like set_params it leaves the frozen state and clears an fp8 calibration."""
        self._sync_stream()
        L.check(L.lib.fcn8s_ema_swap(self.h), self.h)

    @contextlib.contextmanager
    def averaged_weights(self):
        """with engine.averaged_weights(): ... -- the averaged weights are live inside the block, the raw ones again behind it, whatever
        the block raises.  Without a shadow the block runs on the parameters as they are; inside another such block it changes nothing."""
        info = self.ema_info()
        if not info['has_shadow'] or info['swapped']:
            yield self
            return
        self.ema_swap()
        try:
            yield self
        finally:
            self.ema_swap()

    @property
    def pending_micro_batches(self):
        """Micro-batches accumulated (accumulate_step) and not yet applied by a train_step."""
        return int(L.lib.fcn8s_accumulate_pending(self.h))

    def discard_accumulated(self):
        """Forget the accumulated micro-batches (the accumulator's memory stays)."""
        L.check(L.lib.fcn8s_accumulate_discard(self.h), self.h)

    def accumulate_step(self, images, labels, keep_prob=0.5, l2_rate=0.0, fetch_loss=True):
        """One micro-batch that is not the last of its update: forward, backward, and every gradient bucket folded into the model's
        accumulator (fcn8s_accumulate_bucket).  No exchange, no update, the global step stays.  The train_step that follows is the
        last micro-batch: it adds the accumulated gradients to its own in front of each bucket's exchange and divides its gradient
        scale by the number of micro-batches.  Returns the micro-batch's loss (None without fetch_loss)."""
        self._sync_stream()
        ka, pi, dt, pl, where, nhw = self._inputs(images, labels)
        N, H, W = (int(x) for x in nhw)
        self._loss_shape = (N, H, W)
        L.check(L.lib.fcn8s_forward_loss(self.h, pi, dt, pl, N, H, W, float(keep_prob), float(l2_rate), where), self.h)
        self._release(ka)
        self._soft_targets = None                          # (a binding is consumed by the loss that has just been queued)
        for b in range(self.num_buckets):
            L.check(L.lib.fcn8s_backward_bucket(self.h, b), self.h)
            L.check(L.lib.fcn8s_accumulate_bucket(self.h, b, 0), self.h)
        if not fetch_loss:
            return None
        loss = C.c_float(0.0)
        L.check(L.lib.fcn8s_read_loss(self.h, C.byref(loss)), self.h)
        return float(loss.value)

    def train_step(self, images, labels, learning_rate, keep_prob=0.5, l2_rate=0.0,
                   optimizer=L.OPT_TF_ADAM, fetch_loss=True, reduce=True):
        """sess.run([train_op, total_loss, global_step]) (fcn8s_tensorflow.py:554-572).
        `reduce=False` skips the gradient exchange of a data-parallel run (measurement only: bench.py's local-only leg).
        With micro-batches pending (accumulate_step) this is the last one of the update; with a clip set (set_grad_clip) the update is
        clipped.  Both take the split-phase route below; without either the step is what it was."""
        self._sync_stream()
        ka, pi, dt, pl, where, nhw = self._inputs(images, labels)
        N, H, W = (int(x) for x in nhw)
        ws = self.world_size
        loss = C.c_float(0.0)
        always = bool(getattr(self, "dp_always", False)) and _dist() is not None
        pending = self.pending_micro_batches
        if ws == 1 and optimizer == L.OPT_TF_ADAM and not always and not self.native_comm and not pending and self.grad_clip is None:
            step = C.c_int64(0)
            self._loss_shape = (N, H, W)
            L.check(L.lib.fcn8s_train_step(self.h, pi, dt, pl, N, H, W, float(learning_rate), float(keep_prob),
                                           float(l2_rate), where, None, C.byref(step)), self.h)
            self._release(ka)
            self._soft_targets = None
            if fetch_loss:
                L.check(L.lib.fcn8s_read_loss(self.h, C.byref(loss)), self.h)
            return (float(loss.value) if fetch_loss else None), int(step.value)
        trace = getattr(self, "comm_trace", None)          # bench.py: a list collects (step start, per-bucket issue / completion events)
        if trace is not None:                              # t0 in front of the forward pass: the traced times are "ms after the step's first kernel"
            t0 = self.torch.cuda.Event(enable_timing=True); t0.record()
            trace.append(("step", t0, None))
        self._loss_shape = (N, H, W)
        L.check(L.lib.fcn8s_forward_loss(self.h, pi, dt, pl, N, H, W, float(keep_prob), float(l2_rate), where), self.h)
        self._release(ka)
        self._soft_targets = None                          # (a binding is consumed by the loss that has just been queued)
        red = BucketReducer(self.flat_grads, self.buckets, self.pg, trace=trace, always=always, ready=self._bucket_ready)
        # bucket b is final once call b has returned (include/fcn8s_hip.h): {fc7, decoder}, {fc6}, {conv4, conv5}, {conv1 .. conv3}
        # leave in that order, each while the rest of the backward pass runs
        for b in range(self.num_buckets):
            L.check(L.lib.fcn8s_backward_bucket(self.h, b), self.h)
            if pending:                                    # g[b] += acc[b]; the bucket's event moves behind the flush kernel
                L.check(L.lib.fcn8s_accumulate_bucket(self.h, b, 1), self.h)
            if reduce:
                if self.native_comm:
                    L.check(L.lib.fcn8s_allreduce_bucket(self.h, b), self.h)
                else:
                    red.reduce_bucket(b)
        red.wait()
        scale = (1.0 / self.comm_world) if (self.native_comm and reduce) else (red.grad_scale() if reduce else 1.0)
        if pending:
            scale = scale / (pending + 1)
        L.check(L.lib.fcn8s_apply_update(self.h, optimizer, float(learning_rate), scale), self.h)     # (waits for the native all-reduces itself)
        if trace is not None:
            t1 = self.torch.cuda.Event(enable_timing=True); t1.record()
            trace.append(("end", t1, None))
        if fetch_loss:
            L.check(L.lib.fcn8s_read_loss(self.h, C.byref(loss)), self.h)
        step = self.global_step
        every = int(getattr(self, "replica_check_every", 0) or 0)
        if reduce and ws > 1 and every > 0 and step % every == 0:
            self.check_replicas()
        return (float(loss.value) if fetch_loss else None), step

    def _bucket_ready(self, b):
        """A torch side stream that waits for exactly the last kernel writing into gradient bucket b (fcn8s_bucket_wait): a collective
        issued with that stream current starts when the bucket is final, not when everything queued behind it has run."""
        torch = self.torch
        if self._side is None:
            self._side = [torch.cuda.Stream(device=self.device) for _ in range(self.num_buckets)]
        st = self._side[b]
        L.check(L.lib.fcn8s_bucket_wait(self.h, b, C.c_void_p(st.cuda_stream)), self.h)
        return st

    def comm_init_native(self, unique_id=None, rank=None, world=None):
        """Give this model a RCCL rank of its own inside libfcn8s_hip.so (fcn8s_comm_init): from then on train_step exchanges the gradient
        buckets through fcn8s_allreduce_bucket instead of torch.distributed.  Without arguments the unique id is made by rank 0 of the
        current torch.distributed group and handed round through it (any backend: the group only carries 128 bytes, once)."""
        d = _dist()
        if unique_id is None:
            rank = d.get_rank(self.pg) if d else 0
            world = d.get_world_size(self.pg) if d else 1
            buf = C.create_string_buffer(L.COMM_ID_BYTES)
            if rank == 0:
                L.check(L.lib.fcn8s_comm_unique_id(buf, L.COMM_ID_BYTES))
            if d and world > 1:
                box = [bytes(buf.raw)]
                d.broadcast_object_list(box, src=d.get_global_rank(self.pg, 0) if self.pg is not None else 0, group=self.pg)
                buf = C.create_string_buffer(box[0], L.COMM_ID_BYTES)
            unique_id = buf.raw
        self._sync_stream()
        L.check(L.lib.fcn8s_comm_init(self.h, unique_id, len(unique_id), int(rank), int(world)), self.h)
        self.native_comm, self.comm_world, self.comm_rank = True, int(world), int(rank)
        return unique_id

    def comm_destroy(self):
        """fcn8s_comm_destroy: give the library's RCCL rank back; train_step exchanges through torch.distributed again (or not at all).
        Raises with RCCL's / the watchdog's text if the communicator had failed (a dead or hung peer: include/fcn8s_hip.h)."""
        self._sync_stream()
        self.native_comm, self.comm_world, self.comm_rank = False, 1, 0
        L.check(L.lib.fcn8s_comm_destroy(self.h), self.h)

    def comm_info(self):
        r, w, v = C.c_int(), C.c_int(), C.c_int()
        L.check(L.lib.fcn8s_comm_info(self.h, C.byref(r), C.byref(w), C.byref(v)), self.h)
        return {"rank": r.value, "world": w.value, "rccl_version": v.value}

    def check_replicas(self):
        """Data-parallel guard (dp.check_replicas): every rank must hold the same global step and the same bits in a sample of the
        parameters (the sample moves with the step; replicas are identical by construction, this catches the day they are not)."""
        from .dp import check_replicas          # (the library works on torch's current stream: the reads below are ordered behind the update)
        return check_replicas(self.flat_params, self.global_step, self.pg)

    def forward_backward(self, images, labels, keep_prob=1.0, l2_rate=0.0):
        """Gradients only (no update): returns the loss; gradients via get_grads()/grad_view()."""
        self._sync_stream()
        ka, pi, dt, pl, where, nhw = self._inputs(images, labels)
        N, H, W = (int(x) for x in nhw)
        self._loss_shape = (N, H, W)
        L.check(L.lib.fcn8s_forward_loss(self.h, pi, dt, pl, N, H, W, float(keep_prob), float(l2_rate), where), self.h)
        self._release(ka)
        self._soft_targets = None                          # (a binding is consumed by the loss that has just been queued)
        for b in range(self.num_buckets):
            L.check(L.lib.fcn8s_backward_bucket(self.h, b), self.h)
        loss = C.c_float(0.0)
        L.check(L.lib.fcn8s_read_loss(self.h, C.byref(loss)), self.h)
        return float(loss.value)

    def apply_update(self, learning_rate, optimizer=L.OPT_TF_ADAM, grad_scale=1.0):
        self._sync_stream()
        L.check(L.lib.fcn8s_apply_update(self.h, optimizer, float(learning_rate), float(grad_scale)), self.h)

    def eval_step(self, images, labels, l2_rate=0.0):
        """sess.run(metric_update_ops) (fcn8s_tensorflow.py:685-689), keep_prob = 1."""
        self._sync_stream()
        ka, pi, dt, pl, where, nhw = self._inputs(images, labels)
        N, H, W = (int(x) for x in nhw)
        L.check(L.lib.fcn8s_eval_step(self.h, pi, dt, pl, N, H, W, float(l2_rate), where), self.h)
        self._release(ka)

    def metrics_reset(self):
        self._sync_stream()
        L.check(L.lib.fcn8s_metrics_reset(self.h), self.h)

    def _metrics_raw_padded(self):
        Cn = self.num_classes
        cm = np.zeros((Cn, Cn), np.int64); ls = C.c_double(); lc = C.c_int64()
        L.check(L.lib.fcn8s_metrics_raw(self.h, cm.ctypes.data_as(C.c_void_p), C.byref(ls), C.byref(lc)), self.h)
        return cm, float(ls.value), int(lc.value)

    def metrics_raw(self):
        """(confusion matrix [label, prediction] over the caller's classes, sum of the per-batch losses, number of batches)"""
        cm, ls, lc = self._metrics_raw_padded()
        c = self.logical_classes
        return np.ascontiguousarray(cm[:c, :c]), ls, lc

    def metrics_allreduce(self):
        """Sum the confusion matrix and the per-batch loss samples over ranks."""
        if self.native_comm:
            self._sync_stream()
            L.check(L.lib.fcn8s_comm_allreduce_metrics(self.h), self.h)
            return
        d = _dist()
        if not d or self.world_size == 1:
            return
        torch = self.torch
        cm, ls, lc = self._metrics_raw_padded()
        t = torch.cat([torch.from_numpy(cm.reshape(-1)).double(), torch.tensor([ls, float(lc)], dtype=torch.float64)]).to(self.device)
        d.all_reduce(t, group=self.pg)
        t = t.cpu()
        cm = t[:-2].round().long().numpy().reshape(cm.shape).astype(np.int64)
        L.check(L.lib.fcn8s_metrics_set_raw(self.h, np.ascontiguousarray(cm).ctypes.data_as(C.c_void_p), float(t[-2]), int(round(float(t[-1])))), self.h)

    def metrics_get(self, all_classes=False):
        """(mean loss, mean IoU, accuracy).  all_classes: average the IoU over all classes, absent ones counting 0 (what the
        tutorial's TF 1.3.0 tf.metrics.mean_iou does) instead of over the classes that occur (later TF 1.x)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.check(L.lib.fcn8s_metrics_get_ex(self.h, C.byref(a), C.byref(b), C.byref(c), 1 if all_classes else 0), self.h)
        if all_classes and self.logical_classes != self.num_classes:      # the padding classes never occur: they must not count as absent ones
            b = C.c_double(b.value * self.num_classes / self.logical_classes)
        return float(a.value), float(b.value), float(c.value)

    def augment(self, images, labels=None, out_hw=None, offsets=None, flips=None, gains=None, void_class_id=0):
        """GPU-side augmentation of a uint8 batch already on the device (not in the reference, whose BatchGenerator augments on
        the host: batch_generator.py:293-379).  images: uint8 cuda tensor [N,H,W,3]; labels: uint8 cuda tensor [N,H,W] or None.
        Per image: `offsets[n] = (y, x)` top-left corner of the output window in the source (negative = place the source inside a
        larger canvas, like `random_crop` does), `flips[n]` horizontal flip, `gains[n]` brightness factor (None / NaN = no brightness step
        for that image; a factor, 1.0 included, runs the reference's 8-bit HSV round trip, which is not the identity).  Bit-exact with
        the host BatchGenerator (cv2_compat.py).  Returns the augmented (images, labels) as new cuda tensors of size `out_hw`."""
        torch = self.torch
        self._sync_stream()
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_cuda:
            raise ValueError("`images` must be a uint8 cuda tensor of shape (N, H, W, 3)")
        N, H, W = (int(x) for x in images.shape[:3])
        Ho, Wo = (int(x) for x in (out_hw or (H, W)))
        par = np.zeros((N, 4), np.int32)
        if offsets is not None:
            par[:, :2] = np.asarray(offsets, np.int32).reshape(N, 2)
        if flips is not None:
            par[:, 2] = np.asarray(flips).astype(np.int32).reshape(N)
        vl = None
        if gains is not None:
            g = np.asarray([np.nan if x is None else x for x in gains], np.float64).reshape(N)
            par[:, 3] = ~np.isnan(g)
            v = np.arange(256, dtype=np.uint8)[None, :] * np.where(np.isnan(g), 1.0, g)[:, None]      # the reference's float64 `hsv[:,:,2] * random_br`
            vl = torch.from_numpy(np.where(v > 255, 255, v).astype(np.uint8)).to(self.device)         # ... saturated, truncated on the uint8 store
        pd = torch.from_numpy(par).to(self.device)
        images = images.contiguous()
        out = torch.empty((N, Ho, Wo, 3), dtype=torch.uint8, device=self.device)
        lab_out = None; lp = lo = None
        if labels is not None:
            if labels.dtype != torch.uint8 or tuple(labels.shape) != (N, H, W) or not labels.is_cuda:
                raise ValueError("`labels` must be a uint8 cuda tensor of shape (N, H, W)")
            labels = labels.contiguous()
            lab_out = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=self.device)
            lp, lo = C.c_void_p(labels.data_ptr()), C.c_void_p(lab_out.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib.fcn8s_op_augment_u8(stream, C.c_void_p(images.data_ptr()), lp, C.c_void_p(out.data_ptr()), lo,
                                          C.c_void_p(pd.data_ptr()), C.c_void_p(vl.data_ptr()) if vl is not None else None,
                                          N, H, W, Ho, Wo, int(void_class_id)))
        return out, lab_out

    def resample(self, images, labels=None, out_hw=None, sizes=None, offsets=None, void_class_id=0):
        """GPU-side resize / scale / translate of a uint8 batch already on the device (fcn8s_op_resample_u8; the reference's
        BatchGenerator does these on the host, batch_generator.py:328-384).  images: uint8 cuda tensor [N,H,W,3]; labels: uint8 cuda
        tensor [N,H,W] or None.  Per image: `sizes[n] = (rh, rw)` size the source is resized to (default: out_hw), `offsets[n] =
        (oy, ox)` where its top-left corner lands in the output (negative = crop).  Images follow cv2.resize(INTER_LINEAR), labels
        cv2.resize(INTER_NEAREST), bit-exact with the host BatchGenerator (cv2_compat.py).  Returns new (images, labels) of size out_hw."""
        torch = self.torch
        self._sync_stream()
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_cuda:
            raise ValueError("`images` must be a uint8 cuda tensor of shape (N, H, W, 3)")
        N, H, W = (int(x) for x in images.shape[:3])
        Ho, Wo = (int(x) for x in (out_hw or (H, W)))
        par = np.zeros((N, 4), np.int32)
        par[:, :2] = np.asarray(sizes, np.int32).reshape(N, 2) if sizes is not None else (Ho, Wo)
        if offsets is not None:
            par[:, 2:] = np.asarray(offsets, np.int32).reshape(N, 2)
        pd = torch.from_numpy(par).to(self.device)
        images = images.contiguous()
        out = torch.empty((N, Ho, Wo, 3), dtype=torch.uint8, device=self.device)
        lab_out = None; lp = lo = None
        if labels is not None:
            if labels.dtype != torch.uint8 or tuple(labels.shape) != (N, H, W) or not labels.is_cuda:
                raise ValueError("`labels` must be a uint8 cuda tensor of shape (N, H, W)")
            labels = labels.contiguous()
            lab_out = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=self.device)
            lp, lo = C.c_void_p(labels.data_ptr()), C.c_void_p(lab_out.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(L.lib.fcn8s_op_resample_u8(stream, C.c_void_p(images.data_ptr()), lp, C.c_void_p(out.data_ptr()), lo,
                                           C.c_void_p(pd.data_ptr()), N, H, W, Ho, Wo, int(void_class_id)))
        return out, lab_out

    def _alloc_out(self, shape, dtype, where):
        """An uninitialised output where the call's inputs are -- a torch tensor on the device, a numpy array on the host -- and the pointer to pass."""
        if where == L.DEVICE:
            t = self.torch.empty(shape, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)
            return t, C.c_void_p(t.data_ptr())
        a = np.empty(shape, dtype)
        return a, a.ctypes.data_as(C.c_void_p)

    def _predict_out(self, nhw, argmax, where):
        """A prediction's output: int64 [N,H,W] (argmax) or float32 [N,H,W,num_classes], as `_alloc_out`."""
        return self._alloc_out(nhw, np.int64, where) if argmax else self._alloc_out(nhw + (self.num_classes,), np.float32, where)

    def _trim_classes(self, out, argmax):
        """A prediction without the padded classes (`logical_classes` < `num_classes`)."""
        if argmax or self.logical_classes == self.num_classes:
            return out
        out = out[..., :self.logical_classes]
        return np.ascontiguousarray(out) if isinstance(out, np.ndarray) else out.contiguous()

    def predict(self, images, argmax=True):
        """sess.run(predictions_argmax | softmax_output) (fcn8s_tensorflow.py:764-770)."""
        self._sync_stream()
        if isinstance(images, Staged):
            ka_i, pi, dt, _, where, nhw = self._inputs(images, None)
        else:
            ka_i, pi, dt, where, nhw = self._images(images)
        N, H, W = (int(x) for x in nhw)
        out, po = self._predict_out((N, H, W), argmax, where)
        L.check(L.lib.fcn8s_predict(self.h, pi, dt, N, H, W, int(bool(argmax)), po, where), self.h)
        self._release(ka_i)
        return self._trim_classes(out, argmax)

    # ---- fp8_infer calibration (include/fcn8s_hip.h: fcn8s_fp8_calibrate) ---------------------------------------------------
    def calibrate_fp8(self, images, reset=False):
        """In the 'fp8_infer' precision: run the fp32 forward pass on `images` and fold each FP8 layer's max |input| into the calibration
        (reset=True starts over).  Returns the calibration (`fp8_calibration()`)."""
        self._sync_stream()
        ka_i, pi, dt, where, nhw = self._images(images)
        N, H, W = (int(x) for x in nhw)
        L.check(L.lib.fcn8s_fp8_calibrate(self.h, pi, dt, N, H, W, where, int(bool(reset))), self.h)
        del ka_i
        return self.fp8_calibration()

    def fp8_calibration(self):
        """The FP8 calibration, float32[14] (the max |input| of conv1_2 .. conv5_3, fc6, fc7), or None if the model has none."""
        a = np.empty(L.FP8_LAYERS, np.float32)
        rc = L.lib.fcn8s_fp8_get_calibration(self.h, a.ctypes.data_as(L._fp), a.size)
        if rc == L.ERR_STATE:
            return None
        L.check(rc, self.h)
        return a

    def set_fp8_calibration(self, amax):
        a = np.ascontiguousarray(np.asarray(amax, dtype=np.float32).reshape(-1))
        if a.size != L.FP8_LAYERS:
            raise ValueError("an FP8 calibration has %d maxima, got %d" % (L.FP8_LAYERS, a.size))
        L.check(L.lib.fcn8s_fp8_set_calibration(self.h, a.ctypes.data_as(L._fp), a.size), self.h)

    def predict_tta(self, images, scales=(1.0,), flip=False, argmax=True):
        """Multi-scale / left-right-flip prediction on images of any size (fcn8s_predict_tta; the pass rule is in tta.py): the mean over
        the passes of the softmax resized to the input size, or its argmax.  Host or device inputs and outputs, as `predict`."""
        sc = tta.validate(scales, flip)
        self._sync_stream()
        ka_i, pi, dt, where, nhw = self._images(images)
        N, H, W = (int(x) for x in nhw)
        if dt == L.IMG_F32 and tta.resizes(H, W, sc):
            raise ValueError("float32 images are taken only when no pass resizes them; pass uint8 images to predict at scales %s" % (sc,))
        arr = (C.c_float * len(sc))(*sc)
        out, po = self._predict_out((N, H, W), argmax, where)
        L.check(L.lib.fcn8s_predict_tta(self.h, pi, dt, N, H, W, arr, len(sc), int(bool(flip)), int(bool(argmax)), po, where), self.h)
        self._release(ka_i)
        return self._trim_classes(out, argmax)

    def predict_mc(self, images, samples=20, keep_prob=0.5, sample_offset=0, argmax=True, entropy=True, mutual_information=True):
        """Monte-Carlo dropout inference (fcn8s_predict_mc; the definition is in mc_dropout.py): `samples` stochastic passes with dropout
        on behind fc6 and fc7 at `keep_prob` -- the encoder runs once, fc6 -> fc7 -> decoder once per sample -- and the mean of their
        softmaxes.  Returns (prediction, entropy | None, mutual_information | None): the mean softmax float32 [N,H,W,C] or (argmax) its
        int64 argmax [N,H,W]; the predictive entropy of the mean and the mutual information between prediction and weights, float32
        [N,H,W].  Sample s of the call draws its masks on the counter streams mc_dropout.stream_ids(sample_offset, s).  Images of any
        size; host or device inputs and outputs, as `predict`."""
        S, keep, off = mc_dropout.validate(samples, keep_prob, sample_offset)
        self._sync_stream()
        ka_i, pi, dt, where, nhw = self._images(images)
        N, H, W = (int(x) for x in nhw)
        out, po = self._predict_out((N, H, W), argmax, where)
        ent, pe = self._alloc_out((N, H, W), np.float32, where) if entropy else (None, None)
        mi, pm = self._alloc_out((N, H, W), np.float32, where) if mutual_information else (None, None)
        L.check(L.lib.fcn8s_predict_mc(self.h, pi, dt, N, H, W, S, keep, off, int(bool(argmax)), po, pe, pm, where), self.h)
        self._release(ka_i)
        return self._trim_classes(out, argmax), ent, mi

    def predict_crf(self, images, crf, scales=(1.0,), flip=False, argmax=True):
        """`predict_tta` with these arguments followed by a mean-field CRF on its mean softmax and the uint8 images (fcn8s_predict_crf; the
        definition and the parameters are in crf.py): Q^T float32 [N,H,W,C], or its argmax.  `crf`: True for the defaults, a dict of fields
        or a crf.Params; None / False (or iterations = 0) is `predict_tta` itself.  Host or device inputs and outputs, as `predict`."""
        params = crf_mod.resolve(crf)
        if params is None:
            return self.predict_tta(images, scales=scales, flip=flip, argmax=argmax)
        sc = tta.validate(scales, flip)
        self._sync_stream()
        ka_i, pi, dt, where, nhw = self._images(images)
        N, H, W = (int(x) for x in nhw)
        if dt == L.IMG_F32 and params.iterations > 0:
            raise ValueError("the CRF reads the colours of the uint8 images; float32 images are not taken with iterations > 0")
        if dt == L.IMG_F32 and tta.resizes(H, W, sc):
            raise ValueError("float32 images are taken only when no pass resizes them; pass uint8 images to predict at scales %s" % (sc,))
        arr = (C.c_float * len(sc))(*sc)
        cp = L.CrfParams(**params.as_dict())
        out, po = self._predict_out((N, H, W), argmax, where)
        L.check(L.lib.fcn8s_predict_crf(self.h, pi, dt, N, H, W, arr, len(sc), int(bool(flip)), C.byref(cp), int(bool(argmax)), po, where), self.h)
        self._release(ka_i)
        return self._trim_classes(out, argmax)

    def reliability_pair(self, prob, gt, lut, scores=(), scales=(), bins=15, tables=None):
        """One `fcn8s_op_reliability_pair` call (reliability.py; the definition is in include/fcn8s_hip.h) on device tensors: `prob` float32
        [N,H,W,C] as `predict(argmax=False)`, `predict_tta`, `predict_crf` and `predict_mc` return it, `gt` uint8 [N,H,W], `lut` 256 uint8
        (true class = lut[gt]; 255 = ignore), up to 3 float32 uncertainty maps [N,H,W] with their scales.  The counts are accumulated into
        `tables` (calib, sums, hist, bad: int64 device tensors; None makes zeroed ones), which stay on the device and are returned."""
        from . import reliability
        return reliability.counts_device(prob, gt, lut, scores=scores, scales=scales, bins=bins, tables=tables)

    def temperature_nll(self, prob, gt, lut, betas, tables=None):
        """One `fcn8s_op_temperature_nll` call (temperature.py; the definition is in include/fcn8s_hip.h) on device tensors: the NLL of `prob`
        (float32 [N,H,W,C], as the predict routes return it with argmax=False) calibrated at each of the up to 32 `betas` = 1 / T (host values)
        against `gt` uint8 [N,H,W] through `lut` (true class = lut[gt]; 255 = ignore), accumulated into `tables` (int64 [K + 3] on the device:
        nll [K], count, bad [2]; None makes a zeroed one), which stays on the device and is returned."""
        from . import temperature
        return temperature.nll_device(prob, gt, lut, betas, tables=tables)

    def temperature_apply(self, prob, temperature, entropy=False, out=None):
        """One `fcn8s_op_temperature_apply` call: `prob` (float32 [N,H,W,C]) calibrated at `temperature`.  A device tensor: into `out` (None: a
        new tensor; `prob` itself: in place; False: not written); a host array is uploaded, and the results come back as arrays.  Returns
        (calibrated | None, entropy | None): with `entropy`, the entropy [N,H,W] of the calibrated distribution from the same launch."""
        from . import temperature as ts
        torch = self.torch
        if isinstance(prob, torch.Tensor):
            return ts.apply_device(prob, temperature, entropy=entropy, out=out)
        dev = torch.from_numpy(np.ascontiguousarray(prob, dtype=np.float32)).to(self.device)
        q, h = ts.apply_device(dev, temperature, entropy=entropy, out=False if out is False else dev)
        return (None if q is None else q.cpu().numpy()), (None if h is None else h.cpu().numpy())

    def pseudo_label(self, prob, thresholds=None, out_ids=None, ignore_id=255, base=None, base_fill=None, score=None, score_max=None, labels=True,
                     tables=None):
        """One `fcn8s_op_pseudo_label` call (pseudo_label.py; the definition is in include/fcn8s_hip.h) on device tensors, on the current
        stream: `prob` float32 [N,H,W,C] as `predict(argmax=False)`, `predict_tta`, `predict_crf` and `predict_mc` return it (the padded
        classes already trimmed, as for `reliability_pair`); per class a threshold and the label to write (None: 0 and the class itself);
        `base` uint8 [N,H,W] labels to complete where they equal `base_fill`; `score` float32 [N,H,W] gated at `score_max`.  Returns
        (labels uint8 [N,H,W] with `ignore_id` where a pixel is not kept, or None with labels=False; tables), `tables` a dict of the int64
        device tensors hist [C,1024] (None in it: not kept), counts [C,2], misc [3] that are accumulated into -- None makes zeroed ones."""
        from . import pseudo_label
        return pseudo_label.labels_device(prob, thresholds=thresholds, out_ids=out_ids, ignore_id=ignore_id, base=base, base_fill=base_fill,
                                          score=score, score_max=score_max, labels=labels, tables=tables)

    def class_mix(self, images, labels, src=None, seed=0, draw=0, num_classes=None, status=False, selected=False):
        """One `fcn8s_op_class_mix` call (class_mix.py; the definition is in include/fcn8s_hip.h) on uint8 device tensors [N,H,W,3] and
        [N,H,W], on the current stream: for destination n, half of the classes present in image src[n] (None: (n + 1) mod N) are pasted onto
        image n, pixels and labels alike; the choice is a function of (`seed`, `draw`, n).  `num_classes` None: the model's.  The scratch is
        kept on the engine and regrown only when a larger one is needed.  Returns new tensors (images, labels), followed by the uint8
        [N, 256] table of selected classes with `selected`, and by the flag (1: a src[n] lay outside [0, N) and counted as n) with `status`,
        which synchronises and is meant for tests."""
        from . import class_mix
        out_i, out_l, sel, self._class_mix_work = class_mix.mix_device(
            images, labels, src=src, seed=seed, draw=draw, num_classes=self.logical_classes if num_classes is None else num_classes,
            selected=selected, work=getattr(self, "_class_mix_work", None))
        res = (out_i, out_l) + ((sel,) if selected else ())
        if status:
            res += (class_mix.flag_of(self._class_mix_work, labels.shape[0]),)
        return res

    def strong_augment(self, images, seed=0, draw=0, jitter=None, blur=None, params=False):
        """One `fcn8s_op_strong_augment` call (strong_augment.py; the definition is in include/fcn8s_hip.h) on a uint8 device tensor
        [N,H,W,3], on the current stream: per image a gated colour jitter (`jitter` = five ints {gate, contrast, saturation, brightness,
        hue}, None: none) and a gated Gaussian blur (`blur` = (gate, taps [Q, R + 1]) with `strong_augment.taps_table`'s taps, None: none);
        the draws are a function of (`seed`, `draw`, n) with `class_mix`'s counters.  The small arrays travel in the launch arguments:
        nothing is uploaded and nothing synchronises.  The scratch is kept on the engine and regrown only when a larger one is needed.
        Returns a new tensor, with `params` (images, int32 [N, 8] = {colour step ran, c16, s16, b16, dh, m, blur ran, q} per image)."""
        from . import strong_augment
        out, par, self._strong_augment_work = strong_augment.augment_device(
            images, seed=seed, draw=draw, jitter=jitter, blur=blur, params=params, work=getattr(self, "_strong_augment_work", None))
        return (out, par) if params else out

    def fda_transfer(self, images, targets, b=None, beta=0.01, pair=None, out_float=False, status=False):
        """One `fcn8s_op_fda_transfer` call (fda.py; the definition is in include/fcn8s_hip.h) on uint8 device tensors [N,H,W,3] and [M,H,W,3]
        of one height and width, on the current stream: Fourier domain adaptation -- the amplitudes of the (2 b + 1)^2 lowest frequencies of
        source n become those of target pair[n] (None: n mod M; a sequence of N ints in [0, M); or an int32 device tensor of N), the phases
        stay.  `b` None: `fda.half_width(H, W, beta)` = floor(min(H, W) beta), the published rule.  The scratch is kept on the engine and
        regrown only when a larger one is needed.  Returns a new tensor, uint8 (clamp(rint(y), 0, 255)) or, with `out_float`, the float32 y;
        followed by the flag (1: a pair[n] of a device tensor lay outside [0, M) and counted as n mod M) with `status`, which synchronises
        and is meant for tests."""
        from . import fda
        if b is None:
            if not hasattr(images, "shape") or len(images.shape) != 4:
                raise ValueError("images have to be a contiguous uint8 tensor [N,H,W,3] on the GPU")
            if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not 0.0 <= float(beta) <= 0.5:
                raise ValueError("`beta` must be a number in [0, 0.5], got {!r}".format(beta))
            b = fda.half_width(images.shape[1], images.shape[2], beta)
        out, self._fda_work = fda.transfer_device(images, targets, b, pair=pair, out_float=out_float, work=getattr(self, "_fda_work", None))
        return (out, fda.flag_of(self._fda_work)) if status else out

    def regions_label(self, labels, connectivity=4, area=True):
        """One `fcn8s_op_regions_label` call (regions.py; the definition is in include/fcn8s_hip.h) on a device tensor of class ids, int64 as
        `predict` returns them or uint8, [H,W] or [N,H,W]: (comp, area | None), int32 device tensors of the same shape -- the id (smallest
        pixel index, per image) and the pixel count of every pixel's connected component under `connectivity` (4 or 8)."""
        from . import regions
        comp, ar, self._regions_work = regions.label_device(labels, connectivity=connectivity, area=area, work=getattr(self, "_regions_work", None))
        return comp, ar

    def regions_clean(self, labels, min_area, connectivity=4, rounds=1, stats=False):
        """One `fcn8s_op_regions_clean` call, in place, on a device tensor of class ids (int64 or uint8, [H,W] or [N,H,W]): `rounds` rounds in
        which every component smaller than `min_area` (an int, or a table of 256 per class, 0 = never) takes the class of its largest
        4-adjacent neighbour that is not small.  The scratch is kept on the engine and regrown only when a larger one is needed.  Returns
        the int64 [rounds, 4] stats (components, small, relabelled, pixels changed) as a device tensor when `stats`, else None."""
        from . import regions
        st, self._regions_work = regions.clean_device(labels, min_area, connectivity=connectivity, rounds=rounds, stats=stats,
                                                      work=getattr(self, "_regions_work", None))
        return st

    def panoptic_pair(self, pred, inst, connectivity=4):
        """The segment pair table of panoptic quality (panoptic.py; the definition is in include/fcn8s_hip.h) of a device tensor of class ids
        (int64 train ids as `predict` returns them, or uint8 label ids; [H,W] or [N,H,W]) against the uint16 instance map `inst` (a 16-bit
        device tensor or a NumPy map): one `fcn8s_op_regions_label` and one `fcn8s_op_panoptic_pair` call.  Returns (list of int64 rows
        (kp, kg, pixels) per image in ascending order, int64 array of bad pixels per image).  The scratch is kept on the engine and regrown
        only when a larger one is needed."""
        from . import panoptic
        rows, bad, self._panoptic_work = panoptic.pair_rows_device(pred, inst, connectivity=connectivity, work=getattr(self, "_panoptic_work", None))
        return rows, bad

    def instance_pair(self, prob, labels, comp, inst=None):
        """The instance pair table of instance-level AP (instances.py; the definition is in include/fcn8s_hip.h) of device tensors: `prob`
        float32 [N,H,W,C] (or [H,W,C]) as `predict(argmax=False)` and its siblings return it, `labels` uint8 train ids [N,H,W] -- the class
        every pixel ended up with --, `comp` int32, `regions_label` of that map, and the uint16 instance map `inst` (a 16-bit device tensor,
        a NumPy map, or None: no ground truth, the export route): one `fcn8s_op_instance_pair` call.  Returns (list of int64 rows (kp, v,
        pixels, sum of confidence terms) per image in ascending order, int64 array [N, 2] of pixels with a label >= 20 and with a
        probability outside [0, 1]).  The scratch is kept on the engine and regrown only when a larger one is needed; a hash table or a
        row buffer that the op reports as too small is doubled and the call repeated."""
        from . import instances
        rows, bad, self._instance_work = instances.pair_rows_device(prob, labels, comp, inst, work=getattr(self, "_instance_work", None))
        return rows, bad

    # ---- introspection (tests, bench) -----------------------------------------------------------
    def activation(self, name, shape, missing_ok=False):
        """fcn8s_get_activation.  A conv whose output transform was fused with the next conv's input transform (option `fuse_out_in`)
        has no activation tensor; the library says so (Fcn8sError), or, with `missing_ok`, this returns None."""
        a = np.empty(shape, np.float32)
        rc = L.lib.fcn8s_get_activation(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size)
        if rc == L.ERR_STATE and missing_ok and b"not materialised" in (L.lib.fcn8s_last_error(self.h) or b""):
            return None
        L.check(rc, self.h)
        return a

    def relu_branches(self, nhw):
        """Which ReLU units were on in the last forward pass: {name: bool array (N,h,w,c)} for the convs that feed another conv, each
        block's pool (a block's last conv is never materialised; max(relu(z)) > 0 says the same for the window's maximum), fc6 and fc7
        (with keep_prob 1).  Parity tests hand these to the checker so that both sides differentiate along the same branches."""
        N, H, W = (int(x) for x in nhw)
        out = OrderedDict()
        h, w = H, W
        for b, nconv in enumerate((2, 2, 3, 3, 3), start=1):
            for i in range(1, nconv):
                name = "conv%d_%d" % (b, i)
                try:
                    out[name] = self.activation(name, (N, h, w, self.widths[b - 1])) > 0
                except L.Fcn8sError:          # not materialised (its output transform wrote the next conv's input transform directly): the ReLU record
                    rec = np.empty((N, h, w, self.widths[b - 1]), np.uint8)
                    L.check(L.lib.fcn8s_get_relu_record(self.h, name.encode(), rec.ctypes.data_as(C.c_void_p), rec.size), self.h)
                    out[name] = rec.astype(bool)
            h //= 2; w //= 2
            out["pool%d" % b] = self.activation("pool%d" % b, (N, h, w, self.widths[b - 1])) > 0
        out["fc6"] = self.activation("fc6", (N, h, w, self.widths[5])) > 0
        out["fc7"] = self.activation("fc7", (N, h, w, self.widths[6])) > 0
        return out

    def pool_routes(self, nhw):
        """Where the last training forward/backward pass routes each max-pool gradient: {"pool<b>": uint8 (N,h/2,w/2,c)}, 0..3 = window
        element (2*row + col), 4 = ReLU off (include/fcn8s_hip.h: fcn8s_get_pool_routing).  For the parity checker."""
        N, H, W = (int(x) for x in nhw)
        out = OrderedDict()
        for b in range(1, 6):
            a = np.empty((N, H >> b, W >> b, self.widths[b - 1]), np.uint8)
            L.check(L.lib.fcn8s_get_pool_routing(self.h, b, a.ctypes.data_as(C.c_void_p), a.size), self.h)
            out["pool%d" % b] = a
        return out

    def dropout_masks(self, shape6, shape7):
        m6 = np.empty(shape6, np.float32); m7 = np.empty(shape7, np.float32)
        L.check(L.lib.fcn8s_get_dropout_masks(self.h, m6.ctypes.data_as(C.c_void_p), m6.size, m7.ctypes.data_as(C.c_void_p), m7.size), self.h)
        return m6, m7

    def profile(self, on=True):
        L.check(L.lib.fcn8s_profile_enable(self.h, int(on)), self.h)     # 2 = per-layer groups

    def profile_reset(self):
        L.check(L.lib.fcn8s_profile_reset(self.h), self.h)

    def profile_results(self):
        out = OrderedDict()
        for g in range(L.lib.fcn8s_profile_num_groups(self.h)):
            name = C.c_char_p(); ms = C.c_double(); n = C.c_int64(); fl = C.c_double(); by = C.c_double()
            L.check(L.lib.fcn8s_profile_get(self.h, g, C.byref(name), C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), self.h)
            out[name.value.decode()] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
        return out
