"""Who frees what: every device buffer the library allocates has an owner (csrc/device_buffer.h), and the owners keep a process-wide count of
the bytes they hold (fcn8s_get_option(NULL, "device_bytes_live")).  An engine that has walked through every lazily allocated buffer family and
was then destroyed, and every op-level entry point that allocates scratch, must leave that count where it was -- exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import _lib as L  # noqa: E402
from fcn8s_tensorflow_amd.engine import Engine  # noqa: E402

# the smallest model every precision accepts (bf16_train / fp8_infer: widths % 64, the bf16 modes: fc6 / fc7 % 128) on the smallest batch that still
# gives every buffer family a non-empty member
WIDTHS = (64, 64, 128, 256, 256, 256, 128)
CLASSES, N, H, W = 20, 2, 64, 96


def live():
    v = C.c_int64(-1)
    L.check(L.lib.fcn8s_get_option(None, b"device_bytes_live", C.byref(v)))
    return int(v.value)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def cycle(img, lab):
    """One engine through every buffer family, then destroyed.  Returns the largest count seen on the way."""
    e = Engine(CLASSES, widths=WIDTHS, device_id=0, seed=0)
    e.init_params(seed=1)
    # fp32 training with OHEM (loss_ws) and the Lovász term (lov_ws), keeping every layer's output gradient (kept_dy)
    e.set_option("keep_output_gradients", 1)
    e.set_loss(ohem_thresh=0.7, ohem_min_kept=1000)
    e.set_lovasz(0.5)
    loss, _ = e.train_step(img, lab, 1e-4, keep_prob=0.5)
    assert np.isfinite(loss)
    peak = live()
    # frozen inference: the cached filter banks (u_cache)
    e.freeze(True); e.predict(img); e.predict(img); e.freeze(False)
    # multi-scale + flip (tta_buf, the re-plan path), then the CRF on top of it (crf_buf), then Monte-Carlo dropout (mc_buf)
    e.predict_tta(img, scales=(0.5, 1.0), flip=True)
    e.predict_crf(img, True)
    e.predict_mc(img, samples=2)
    # bf16 forward modes: xbf16, d_wbf16, d_abf16, and frozen the per-layer bf16 kernels (wbf16_cache)
    e.set_precision('bf16_fwd')
    e.train_step(img, lab, 1e-4, keep_prob=0.5)
    e.freeze(True); e.predict(img); e.freeze(False)
    # bf16_train: the guarded copies of every layer's input and output gradient (xg16, dyg16)
    e.set_precision('bf16_train')
    e.train_step(img, lab, 1e-4, keep_prob=0.5)
    e.eval_step(img, lab)
    # fp8_infer: the e4m3 copies (q8), the weight banks (w8), the calibration scratch (d_fp8_amax)
    e.set_precision('fp8_infer')
    e.calibrate_fp8(img, reset=True)
    e.predict(img)
    # the staging slots: stage, wait (inside predict), release
    e.predict(e.stage(img, slot=0))
    peak = max(peak, live())
    e.close()
    return peak


def test_device_memory_returns_to_its_owner_count():
    b0 = live()        # (not necessarily 0: another test's engine may still be alive -- differences only)
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    lab = rng.integers(0, CLASSES, (N, H, W), dtype=np.uint8)
    for rnd in (1, 2):                                    # the second cycle catches what only leaks on reuse
        peak = cycle(img, lab)
        assert peak > b0, "the counter does not count"
        assert live() == b0, (rnd, live() - b0)

    # set_option refuses the key, with or without a model
    assert L.lib.fcn8s_set_option(None, b"device_bytes_live", 0) == L.ERR_BAD_ARG

    # the op-level entry points that allocate scratch (and, the two *_fwd_bwd ones, build a bare model that allocates more behind their back): each at
    # the smallest shape its own parity test uses
    def t(*shape, fill=None):
        return torch.randn(*shape, device='cuda') if fill is None else torch.full(shape, fill, device='cuda')

    def op_winograd(n=1, h=4, w=6, ci=16, co=32, tile=2):
        x, k, b, y = t(n, h, w, ci), t(3, 3, ci, co), t(co), t(n, h, w, co)
        return L.lib.fcn8s_op_conv2d_winograd(None, ptr(x), ptr(k), ptr(b), ptr(y), n, h, w, ci, co, 3, 1, tile)

    def op_wino_fwd_bwd(n, h, w, ci, co, tile, pooled, mask_mode):
        x, k, b = t(n, h, w, ci), t(3, 3, ci, co), t(co)
        dy = t(n, h // 2, w // 2, co) if pooled else t(n, h, w, co)
        y, pool = (None, t(n, h // 2, w // 2, co)) if pooled else (t(n, h, w, co), None)
        sk, dx, dw, db = t(n, h, w, ci), t(n, h, w, ci), t(3, 3, ci, co), t(co)
        return L.lib.fcn8s_op_conv3x3_winograd_fwd_bwd(None, ptr(x), ptr(k), ptr(b), ptr(dy), ptr(sk), ptr(y), ptr(pool), ptr(dx), ptr(dw), ptr(db),
                                                       n, h, w, ci, co, tile, pooled, mask_mode)

    def op_fc6(n=1, h=3, w=3, ci=64, co=128):
        x, k, b, dy = t(n, h, w, ci), t(7, 7, ci, co), t(co), t(n, h, w, co)
        y, dx, dw, db = t(n, h, w, co), t(n, h, w, ci), t(7, 7, ci, co), t(co)
        return L.lib.fcn8s_op_conv7x7_fc6_fwd_bwd(None, ptr(x), ptr(k), ptr(b), ptr(dy), ptr(y), ptr(dx), ptr(dw), ptr(db), n, h, w, ci, co, 2, 1.0, 0, None)

    def op_bf16_train(n=2, h=4, w=4, ci=128, co=256, k=1):
        x, kk, b, dy, mask = t(n, h, w, ci), t(k, k, ci, co), t(co), t(n, h, w, co), t(n, h, w, ci)
        y, dx, dw, db = t(n, h, w, co), t(n, h, w, ci), t(k, k, ci, co), t(co)
        return L.lib.fcn8s_op_conv2d_bf16_train(None, ptr(x), ptr(kk), ptr(b), ptr(y), 1, ptr(dy), ptr(mask), ptr(dx), ptr(dw), ptr(db), n, h, w, ci, co, k)

    def op_fp8(n=1, h=9, w=13, ci=64, co=64, k=3):
        x, kk, b, y = t(n, h, w, ci), t(k, k, ci, co), t(co), t(n, h, w, co)
        return L.lib.fcn8s_op_conv2d_fp8(None, ptr(x), ptr(kk), ptr(b), ptr(y), 1, -6, n, h, w, ci, co, k)

    ops = [("conv2d_winograd", op_winograd),
           ("conv3x3_winograd_fwd_bwd", lambda: op_wino_fwd_bwd(1, 8, 12, 64, 128, 2, 0, 1)),
           # ... and at the smallest shape at which its bare model keeps a forward bank, pool routing bytes and a ReLU bit record
           ("conv3x3_winograd_fwd_bwd, tile 6", lambda: op_wino_fwd_bwd(1, 34, 22, 64, 64, 6, 1, 2)),
           ("conv7x7_fc6_fwd_bwd", op_fc6),
           ("conv2d_bf16_train", op_bf16_train),
           ("conv2d_fp8", op_fp8)]
    for name, op in ops:
        L.check(op())
        torch.cuda.synchronize()
        assert live() == b0, (name, live() - b0)
