"""The Lovász-softmax training loss on the GPU (fcn8s_set_lovasz, fcn8s_get_loss_terms, fcn8s_op_lovasz_softmax; definitions in
include/fcn8s_hip.h, restated in fcn8s_tensorflow_amd/loss.py): the operator against the float64 restatement on the device's own fp32
errors (so the sort order is compared exactly, ties included), at the full bench shape, on logits; the model's loss, terms and last bias
gradient in fp32 and bf16_train; exact linear wiring; per-image shard invariance; determinism and allocation; the facade and errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM
from oracle import fcn8s_oracle as orc

pytestmark = pytest.mark.gpu
SMALL = (8, 16, 32, 64, 64, 128, 128)
W64 = (64, 64, 128, 256, 256, 256, 128)
LAST_BIAS = "fc7_pool4_pool3_conv2d_trans/bias"


def _lib():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run_op(x, lab, nseg, classes_all=0, mask=None, is_logits=0):
    """fcn8s_op_lovasz_softmax on device tensors -> (loss, grad (P, C), class_loss (nseg, C)) as numpy."""
    L = _lib()
    P, Cc = x.shape
    md = torch.tensor(np.asarray(mask, np.uint8)).cuda() if mask is not None else None
    lo = torch.zeros(1).cuda(); g = torch.full((P, Cc), 7.0).cuda(); cl = torch.zeros(nseg * Cc).cuda()
    L.check(L.lib.fcn8s_op_lovasz_softmax(None, ptr(x), int(is_logits), ptr(lab), nseg, P // nseg, Cc, int(classes_all), ptr(md), ptr(lo), ptr(g), ptr(cl)))
    torch.cuda.synchronize()
    return float(lo.cpu()), g.cpu().numpy(), cl.cpu().numpy().reshape(nseg, Cc)


def dev_softmax(logits):
    """The device's fp32 softmax of (P, C) logits (fcn8s_op_softmax_argmax): the probabilities the Lovász kernels use, bit for bit."""
    L = _lib()
    ld = torch.as_tensor(logits).cuda().contiguous()
    P, Cc = ld.shape
    sm = torch.empty(P, Cc).cuda(); am = torch.empty(P, dtype=torch.int64).cuda()
    L.check(L.lib.fcn8s_op_softmax_argmax(None, ptr(ld), ptr(sm), ptr(am), P, Cc))
    torch.cuda.synchronize()
    return sm.cpu().numpy()


def _classes(kind, Cc):
    if kind == "subset":
        ids = list(range(0, Cc, 3))
        m = np.zeros(Cc, np.uint8); m[ids] = 1
        return ids, 1, m
    return kind, int(kind == "all"), None


def _probs_case(P, Cc, seed, quant):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((P, Cc)) * 2
    p = np.exp(z - z.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
    if quant:
        p = np.round(p * 64) / 64                                   # multiples of 1/64: massive ties in the errors
    lab = rng.integers(0, Cc, P).astype(np.uint8)
    lab[rng.random(P) < 0.1] = 255
    lab[:P // 4][lab[:P // 4] == 1] = 255                           # class 1 absent from the first quarter (present mode drops it there)
    return p.astype(np.float32), lab


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("Cc", [4, 12, 20])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", ["present", "all", "subset"])
@pytest.mark.parametrize("quant", [False, True])
def test_op_on_probabilities_exact_order(Cc, per_image, classes, quant):
    N = 4
    p, lab = _probs_case(N * 3000, Cc, Cc * 7 + quant, quant)
    cls, ca, mask = _classes(classes, Cc)
    nseg = N if per_image else 1
    loss, g, cl = run_op(torch.tensor(p).cuda(), torch.tensor(lab).cuda(), nseg, ca, mask)
    r = LM.lovasz_restate(p, lab, N, per_image=per_image, classes=cls, x_is='probs')
    assert abs(loss - r["loss"]) <= 2e-6 * abs(r["loss"]), (loss, r["loss"])
    assert np.abs(cl - r["class_loss"]).max() <= 2e-6 * np.abs(r["class_loss"]).max()
    gp = r["grad_prob"]
    nz = gp != 0
    assert (g[~nz] == 0).all()
    assert (np.abs(g[nz] - gp[nz]) <= 2e-6 * np.abs(gp[nz])).all()          # elementwise: a mis-ordered tie moves g by far more
    assert (g[lab >= Cc] == 0).all()


def _scale_check(p, lab, N, per_image, loss, g, cl):
    """The restatement per segment-class with numpy's stable sort, comparing as it goes (the full float64 planes would not fit)."""
    P, Cc = p.shape
    S = N if per_image else 1
    L = P // S
    total = 0.0
    for s in range(S):
        seg = slice(s * L, (s + 1) * L)
        ls = lab[seg].astype(np.int64)
        valid = np.nonzero(ls < Cc)[0]
        present = [c for c in range(Cc) if (ls[valid] == c).any()]
        segsum = 0.0
        for c in present:
            fg = ls[valid] == c
            pc = p[seg][valid, c]
            e = np.where(fg, (np.float32(1) - pc).astype(np.float32), pc).astype(np.float64)
            order = np.argsort(-e, kind="stable")
            gr = LM.lovasz_grad(fg[order])
            lc = float(np.dot(e[order], gr))
            assert abs(cl[s, c] - lc) <= 2e-6 * lc, (s, c, cl[s, c], lc)
            segsum += lc
            ref = gr * np.sign(pc[order].astype(np.float64) - fg[order]) / (S * len(present))
            got = g[seg][valid[order], c].astype(np.float64)
            assert (np.abs(got - ref) <= 2e-6 * np.abs(ref)).all(), (s, c)
        total += segsum / len(present) if present else 0.0
    assert abs(loss - total / S) <= 2e-6 * (total / S)


@pytest.mark.parametrize("per_image", [False, True])
def test_op_at_bench_scale(per_image):
    N, H, W, Cc = 16, 512, 1024, 20
    gen = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn((N * H * W, Cc), device="cuda", generator=gen) * 2
    x = torch.softmax(z, 1).contiguous()
    lab = torch.randint(0, Cc, (N * H * W,), dtype=torch.uint8, device="cuda", generator=gen)
    lab[torch.rand(N * H * W, device="cuda", generator=gen) < 0.05] = 255
    del z
    loss, g, cl = run_op(x, lab, N if per_image else 1)
    _scale_check(x.cpu().numpy(), lab.cpu().numpy(), N, per_image, loss, g, cl)


@pytest.mark.parametrize("Cc", [4, 12, 20])
@pytest.mark.parametrize("per_image", [False, True])
def test_op_on_logits(Cc, per_image):
    N = 3
    rng = np.random.default_rng(40 + Cc)
    z = (rng.standard_normal((N * 2500, Cc)) * 3).astype(np.float32)
    lab = rng.integers(0, Cc, N * 2500).astype(np.uint8)
    lab[rng.random(N * 2500) < 0.1] = 255
    loss, g, _ = run_op(torch.tensor(z).cuda(), torch.tensor(lab).cuda(), N if per_image else 1, is_logits=1)
    r = LM.lovasz_restate(dev_softmax(z), lab, N, per_image=per_image, x_is='probs')
    assert abs(loss - r["loss"]) <= 2e-6 * r["loss"]
    assert _rel(g, r["grad_logits"]) <= 1e-6


# ---- the model -------------------------------------------------------------------------------------------------------------------
def engine(widths=SMALL, precision="fp32", **opts):
    from fcn8s_tensorflow_amd.engine import Engine
    return Engine(20, widths=widths, device_id=0, seed=0, precision=precision, options=opts)


def model_case(widths, n=2, h=64, w=96, seed=3, ignore=0.1, decoder_std_scale=3.0):
    P = orc.init_params(20, widths, seed=seed, decoder_std_scale=decoder_std_scale, bias_std=0.05)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    lab = rng.integers(0, 20, (n, h, w), dtype=np.uint8)
    lab[rng.random((n, h, w)) < ignore] = 255
    lab[0][lab[0] == 5] = 255                                       # class 5 absent from image 0
    return P, img, lab


def restated_total(logits, lab, n, ce, lov, per_image, classes="present", **loss_cfg):
    rc = LM.restate(logits, lab, **loss_cfg)
    rl = LM.lovasz_restate(dev_softmax(logits), lab, n, per_image=per_image, classes=classes, x_is='probs')
    d = ce * rc["dlogits"] + lov * rl["grad_logits"]
    return dict(loss=ce * rc["loss"] + lov * rl["loss"], ce=rc["loss"], lovasz=rl["loss"], dlogits=d, scale=ce * np.abs(rc["dlogits"]).sum(0).max()
                + lov * np.abs(rl["grad_logits"]).sum(0).max())


@pytest.mark.parametrize("precision,widths", [("fp32", SMALL), ("bf16_train", W64)])
@pytest.mark.parametrize("tconv_gemm", [0, 1])
@pytest.mark.parametrize("per_image", [False, True])
def test_model_matches_restatement(precision, widths, tconv_gemm, per_image):
    P, img, lab = model_case(widths, seed=6)
    n, h, w = lab.shape
    e = engine(widths, precision, tconv_gemm=tconv_gemm)
    e.set_params(P)
    cw = np.random.default_rng(7).uniform(0.5, 2.0, 20).astype(np.float32)
    for ce, lov, loss_cfg in ((1.0, 0.5, {}), (0.0, 1.0, {}), (1.0, 0.5, dict(class_weights=cw, ohem_thresh=0.7, ohem_min_kept=100))):
        e.set_loss(**loss_cfg)
        e.set_lovasz(lov, ce_weight=ce, per_image=per_image)
        loss = e.forward_backward(img, lab, keep_prob=1.0)
        logits = e.activation("logits", (n, h, w, 20)).reshape(-1, 20)
        r = restated_total(logits, lab, n, ce, lov, per_image, **loss_cfg)
        assert abs(loss - r["loss"]) <= 1e-5 * r["loss"], (ce, lov, loss, r["loss"])
        t = e.loss_terms()
        assert abs(t["ce"] - r["ce"]) <= 1e-5 * r["ce"] and abs(t["lovasz"] - r["lovasz"]) <= 1e-5 * r["lovasz"] and t["l2"] == 0.0, (t, r)
        db = e.get_grads()[LAST_BIAS]
        ref = r["dlogits"].sum(0)
        assert np.abs(db - ref).max() <= 1e-5 * r["scale"], (ce, lov, db, ref)
    e.close()


def step_grads(e, P, img, lab, lovasz=None):
    e.set_params(P)
    if lovasz:
        e.set_lovasz(**lovasz)
    loss = e.forward_backward(img, lab, keep_prob=1.0, l2_rate=0.0)
    return loss, {k: v.copy() for k, v in e.get_grads().items()}


def assert_bits(a, b, scale=1.0):
    assert np.float32(a[0]) * np.float32(scale) == np.float32(b[0]), (a[0], b[0])
    assert len(a[1]) == len(b[1]) == 42
    for k in a[1]:
        np.testing.assert_array_equal((a[1][k] * np.float32(scale)).view(np.uint32), b[1][k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("per_image", [False, True])
def test_linear_wiring_is_exact(per_image):
    P, img, lab = model_case(SMALL, seed=4)
    half = step_grads(engine(deterministic=1), P, img, lab, dict(lovasz_weight=0.5, ce_weight=1.0, per_image=per_image))
    dbl = step_grads(engine(deterministic=1), P, img, lab, dict(lovasz_weight=1.0, ce_weight=2.0, per_image=per_image))
    assert_bits(half, dbl, scale=2.0)


def test_reset_and_zero_weight_are_bit_identical_to_a_fresh_engine():
    P, img, lab = model_case(SMALL, seed=5)
    ref = step_grads(engine(deterministic=1), P, img, lab)
    e = engine(deterministic=1)
    step_grads(e, P, img, lab, dict(lovasz_weight=0.7, per_image=True, classes="all"))
    e.set_lovasz(0.0)
    assert e.lovasz_config is None
    assert_bits(ref, step_grads(e, P, img, lab))
    assert e.loss_terms()["lovasz"] == 0.0
    assert_bits(ref, step_grads(engine(deterministic=1), P, img, lab, dict(lovasz_weight=0.0)))


def test_per_image_shards_match_the_big_batch():
    P, img, lab = model_case(SMALL, n=4, seed=8)
    cfg = dict(lovasz_weight=1.0, ce_weight=1.0, per_image=True)
    _, big = step_grads(engine(deterministic=1), P, img, lab, cfg)
    parts = [step_grads(engine(deterministic=1), P, img[i:i + 2], lab[i:i + 2], cfg)[1] for i in (0, 2)]
    for k in big:
        shard = 0.5 * (parts[0][k].astype(np.float64) + parts[1][k])
        assert np.abs(shard - big[k]).max() <= 1e-5 * np.abs(big[k]).max(), k


@pytest.mark.parametrize("per_image", [False, True])
def test_determinism_and_allocation(per_image):
    P, img, lab = model_case(SMALL, seed=10)
    params = []
    for _ in range(2):
        e = engine(deterministic=1)
        e.set_params(P)
        e.set_lovasz(0.5, per_image=per_image)
        e.train_step(img, lab, 1e-3, keep_prob=1.0)
        a = e.get_option("workspace_allocations")
        for _ in range(2):
            loss, _ = e.train_step(img, lab, 1e-3, keep_prob=1.0)
        assert e.get_option("workspace_allocations") == a and np.isfinite(loss)
        params.append({k: v.copy() for k, v in e.get_params().items()})
        e.close()
    for k in params[0]:
        np.testing.assert_array_equal(params[0][k].view(np.uint32), params[1][k].view(np.uint32), err_msg=k)


def gen(n, h, w, seed):
    rng = np.random.default_rng(seed)
    while True:
        img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        lab = rng.integers(0, 19, (n, h, w), dtype=np.uint8)
        yield img, orc.one_hot(lab, 19)


def test_facade_train_and_padding_class():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=19, widths=SMALL)       # 19 classes, padded to the library's 20
    with pytest.raises(ValueError):
        m.train(gen(2, 32, 64, 0), 1, 1, lambda s: 1e-3, lovasz_weight=-1.0)
    with pytest.raises(ValueError):
        m.train(gen(2, 32, 64, 0), 1, 1, lambda s: 1e-3, lovasz_weight=1.0, lovasz_classes=[19])
    m.train(gen(2, 32, 64, 0), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, lovasz_weight=0.5, lovasz_classes='all',
            metrics={'loss'}, eval_frequency=1, record_summaries=False)
    assert m.g_step == 2 and np.isfinite(m.training_loss)
    assert m.engine.lovasz_config is None                                   # restored
    # one more training loss under the same configuration, restated with 19 classes: the padding class never takes part
    e = m.engine
    e.set_lovasz(0.5, classes='all')
    img, oh = next(gen(2, 32, 64, 5))
    lab = oh.argmax(-1).astype(np.uint8)
    loss = e.forward_backward(img, lab, keep_prob=1.0)
    logits = e.activation("logits", (2, 32, 64, 20)).reshape(-1, 20)
    probs = dev_softmax(logits)
    rl = LM.lovasz_restate(probs[:, :19], lab, 2, classes='all', x_is='probs')
    rc = LM.restate(logits, lab)
    t = e.loss_terms()
    assert abs(t["lovasz"] - rl["loss"]) <= 1e-5 * rl["loss"] and abs(t["ce"] - rc["loss"]) <= 1e-5 * rc["loss"]
    assert abs(loss - (rc["loss"] + 0.5 * rl["loss"])) <= 1e-5 * loss
    e.set_lovasz(0.0)


def test_bad_arguments():
    L = _lib()
    e = engine()
    with pytest.raises(Exception):
        e.loss_terms()                                                      # before any training loss: FCN8S_ERR_STATE
    for kw in (dict(lovasz_weight=-1.0), dict(lovasz_weight=float("nan")), dict(lovasz_weight=0.0, ce_weight=0.0),
               dict(lovasz_weight=1.0, classes="none"), dict(lovasz_weight=1.0, classes=[20]), dict(lovasz_weight=1.0, per_image=3)):
        with pytest.raises(ValueError):
            e.set_lovasz(**kw)
    ones = (C.c_uint8 * 20)(*([1] * 20)); zeros = (C.c_uint8 * 20)()
    assert L.lib.fcn8s_set_lovasz(e.h, 1.0, -0.5, 0, 0, ones, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_lovasz(e.h, float("inf"), 0.5, 0, 0, ones, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_lovasz(e.h, 0.0, 0.0, 0, 0, ones, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_lovasz(e.h, 1.0, 0.5, 2, 0, ones, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_lovasz(e.h, 1.0, 0.5, 0, -1, ones, 20) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_lovasz(e.h, 1.0, 0.5, 0, 0, ones, 19) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_set_lovasz(e.h, 1.0, 0.5, 0, 0, zeros, 20) == L.ERR_BAD_ARG
    e.close()
    x = torch.zeros(100, 4).cuda(); lab = torch.zeros(100, dtype=torch.uint8).cuda(); lo = torch.zeros(1).cuda()
    assert L.lib.fcn8s_op_lovasz_softmax(None, ptr(x), 0, ptr(lab), 1, 100, 65, 0, None, ptr(lo), None, None) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_lovasz_softmax(None, ptr(x), 2, ptr(lab), 1, 100, 4, 0, None, ptr(lo), None, None) == L.ERR_BAD_ARG
    assert L.lib.fcn8s_op_lovasz_softmax(None, ptr(x), 0, ptr(lab), 0, 100, 4, 0, None, ptr(lo), None, None) == L.ERR_BAD_ARG
