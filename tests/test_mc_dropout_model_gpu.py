"""Monte-Carlo dropout inference through the model (fcn8s_predict_mc, Engine.predict_mc): without dropout it is `predict` bit for bit;
an S-sample call is the fp32 fold of S one-sample calls (which notices a buffer of the once-run trunk overwritten by the repeated
part); each sample is the network under the masks the library reports, against the oracle; calls are reproducible and leave training's
masks alone; the trunk runs once per call whatever S; and the call leaves the model's state -- allocations, frozen flag, later
predictions -- as it found it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)
from fcn8s_tensorflow_amd import _lib as L, mc_dropout as mc  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)
SMALL64 = (64, 64, 64, 64, 64, 128, 128)        # bf16_train: every width a multiple of 64
FULL = tuple(orc.DEFAULT_WIDTHS)
WIDTHS = {"fp32": SMALL, "bf16_train": SMALL64}

# precision, widths ("small" / "full"), N, H, W, tconv_gemm (the logits in the plain or in the blocked layout)
CASES = [(p, ws, n, h, w, tg)
         for p in ("fp32", "bf16_train")
         for (ws, n, h, w) in (("small", 2, 64, 96), ("small", 1, 128, 128), ("full", 1, 32, 64))      # 128 x 128: a 4 x 4 fc6 map -- fp32 runs it in the transform domain, dropout in the output transform
         for tg in (0, 1)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def params(widths, scale):
    return orc.init_params(20, widths, seed=1, decoder_std_scale=scale, bias_std=0.05)


def widths_of(precision, ws):
    return FULL if ws == "full" else WIDTHS[precision]


def engine(precision="fp32", ws="small", tg=1, seed=77, options=None):
    from fcn8s_tensorflow_amd.engine import Engine
    widths = widths_of(precision, ws)
    opts = {"tconv_gemm": tg}; opts.update(options or {})
    e = Engine(20, widths=widths, device_id=0, seed=seed, precision=precision, options=opts)
    # (bf16_train: the decoder scale test_model_gpu.py's bf16_train cases use, so that their bar applies)
    e.set_params(params(widths, 6.0 if precision == "bf16_train" else 30.0))
    return e


def images(n, h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def ops_bar(logits_per_sample):
    """the ops file's bar: 8 x the largest float32-to-float64 distance of the restatement on these inputs"""
    ref, f32 = mc.restate(logits_per_sample), mc.restate(logits_per_sample, dtype=np.float32)
    return 8.0 * max(float(np.abs(g.astype(np.float64) - r).max()) for r, g in zip(ref[:3], f32[:3]))


def h64(p):
    p = np.asarray(p, np.float64)
    return -(p * np.log(np.maximum(p, mc.FLT_MIN))).sum(-1)


# ---- a. no dropout is `predict` ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,ws,n,h,w,tg", CASES)
def test_without_dropout_it_is_predict(precision, ws, n, h, w, tg):
    e = engine(precision, ws, tg)
    img = images(n, h, w)
    sm = e.predict(img, argmax=False); am = e.predict(img, argmax=True)
    ents = []
    for S in (1, 2, 4):
        p, ent, mi = e.predict_mc(img, samples=S, keep_prob=1.0, argmax=False)
        assert same_bits(p, sm), S
        a, ent2, mi2 = e.predict_mc(img, samples=S, keep_prob=1.0, argmax=True)
        assert same_bits(a, am) and same_bits(ent, ent2) and same_bits(mi, mi2)
        assert (mi == 0.0).all(), (S, float(mi.max()))
        ents.append(ent)
    assert same_bits(ents[0], ents[1]) and same_bits(ents[0], ents[2])
    assert np.abs(ents[0] - h64(sm)).max() < 1e-5 and ents[0].max() > 1e-3
    e.close()


@pytest.mark.parametrize("precision,tg", [("fp32", 1), ("fp32", 0), ("bf16_train", 1)])
def test_without_dropout_any_size_is_predict_tta_at_scale_one(precision, tg):
    e = engine(precision, "small", tg)
    img = images(1, 40, 72)                  # not multiples of 32: padded to 64 x 96
    for S in (1, 2):
        p, ent, mi = e.predict_mc(img, samples=S, keep_prob=1.0, argmax=False)
        assert p.shape == (1, 40, 72, 20) and ent.shape == (1, 40, 72) and mi.shape == (1, 40, 72)
        assert same_bits(p, e.predict_tta(img, scales=(1.0,), argmax=False))
        a, _, _ = e.predict_mc(img, samples=S, keep_prob=1.0, argmax=True)
        assert same_bits(a, e.predict_tta(img, scales=(1.0,), argmax=True))
        assert (mi == 0.0).all()
    # float32 images take the same path
    pf, _, _ = e.predict_mc(img.astype(np.float32), samples=2, keep_prob=1.0, argmax=False)
    assert same_bits(pf, p)
    e.close()


# ---- b. samples compose --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,ws,n,h,w,tg", CASES)
def test_an_s_sample_call_is_the_fold_of_one_sample_calls(precision, ws, n, h, w, tg):
    e = engine(precision, ws, tg)
    img = images(n, h, w)
    o = 5
    singles, logits = [], []
    for k in range(4):
        p, _, _ = e.predict_mc(img, samples=1, keep_prob=0.5, sample_offset=o + k, argmax=False)
        singles.append(p); logits.append(e.activation("logits", (n, h, w, 20)).copy())
    assert not same_bits(singles[0], singles[1]) and not same_bits(singles[1], singles[2])      # other streams, other masks
    mean, ent, mi = e.predict_mc(img, samples=4, keep_prob=0.5, sample_offset=o, argmax=False)
    fold = singles[0].copy()
    for k in range(1, 4):
        fold = fold + singles[k]
    fold = fold * (np.float32(1) / np.float32(4))
    assert fold.dtype == np.float32 and same_bits(mean, fold)
    am, _, _ = e.predict_mc(img, samples=4, keep_prob=0.5, sample_offset=o, argmax=True)
    assert same_bits(am, np.argmax(mean, -1).astype(np.int64))
    # entropy and mutual information: the definition on those four softmaxes, in float64
    bar = ops_bar(np.stack(logits))
    m64 = np.sum([s.astype(np.float64) for s in singles], 0) / 4
    e64 = h64(m64)
    mi64 = np.maximum(0.0, e64 - np.sum([h64(s) for s in singles], 0) / 4)
    d_ent, d_mi = float(np.abs(ent - e64).max()), float(np.abs(mi - mi64).max())
    print("%s %s %dx%dx%d tconv_gemm=%d: bar %.3e, entropy %.3e, mutual information %.3e (max MI %.4f)" % (precision, ws, n, h, w, tg, bar, d_ent, d_mi, float(mi.max())))
    assert d_ent <= bar and d_mi <= bar
    assert mi.max() > 0 and (mi <= ent + bar).all()          # the samples disagree somewhere
    e.close()


# ---- c. each sample is the network with its reported masks ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision,ws,n,h,w,tg", [c for c in CASES if c[5] == 1 or c[1] == "small"])
def test_each_sample_is_the_network_under_its_reported_masks(precision, ws, n, h, w, tg):
    e = engine(precision, ws, tg)
    widths = widths_of(precision, ws)
    P = params(widths, 6.0 if precision == "bf16_train" else 30.0)
    img = images(n, h, w)
    s6, s7 = (n, h // 32, w // 32, widths[5]), (n, h // 32, w // 32, widths[6])
    o = 11
    e.predict_mc(img, samples=1, keep_prob=0.5, sample_offset=o)
    m6, m7 = e.dropout_masks(s6, s7)
    logits = e.activation("logits", (n, h, w, 20))
    assert set(np.unique(m6)) <= {0.0, 1.0} and set(np.unique(m7)) <= {0.0, 1.0}
    if m6.size >= 256:
        assert 0.3 < m6.mean() < 0.7 and 0.3 < m7.mean() < 0.7
    assert not np.array_equal(m6.ravel()[:min(m6.size, m7.size)], m7.ravel()[:min(m6.size, m7.size)])
    ref = orc.forward(P, img, keep_prob=0.5, masks=(m6, m7), bf16_train=(precision == "bf16_train"))
    err, scale = float(np.abs(logits - ref).max()), max(1.0, float(np.abs(ref).max()))
    tol = 2e-2 if precision == "bf16_train" else 1e-4        # the bars tests/test_model_gpu.py holds the two precisions' logits to
    print("%s %s %dx%dx%d tconv_gemm=%d: logits under the reported masks %.3e of the scale (bar %.0e)" % (precision, ws, n, h, w, tg, err / scale, tol))
    assert err < tol * scale, (err / scale, tol)
    assert np.abs(ref - orc.forward(P, img, bf16_train=(precision == "bf16_train"))).max() > 10 * tol * scale or ws == "full"      # the masks matter
    # the next offset has other masks; an S = 3 call that ENDS on the same stream reports the same ones
    e.predict_mc(img, samples=1, keep_prob=0.5, sample_offset=o + 1)
    n6, n7 = e.dropout_masks(s6, s7)
    assert not np.array_equal(n6, m6) and not np.array_equal(n7, m7)
    e.predict_mc(img, samples=3, keep_prob=0.5, sample_offset=o - 2)
    l6, l7 = e.dropout_masks(s6, s7)
    assert same_bits(l6, m6) and same_bits(l7, m7)
    assert same_bits(e.activation("logits", (n, h, w, 20)), logits)          # ... and its last sample IS that sample
    # keep_prob = 1 draws none
    e.predict_mc(img, samples=2, keep_prob=1.0)
    k6, k7 = e.dropout_masks(s6, s7)
    assert (k6 == 1).all() and (k7 == 1).all()
    e.close()


# ---- d. reproducible, offset-dependent, training masks untouched -------------------------------------------------------------------
@pytest.mark.parametrize("precision,tg", [("fp32", 1), ("fp32", 0), ("bf16_train", 1)])
def test_reproducible_and_offset_dependent_and_training_masks_untouched(precision, tg):
    n, h, w = 2, 64, 96
    widths = WIDTHS[precision]
    e = engine(precision, "small", tg, options={"deterministic": 1})
    img = images(n, h, w)
    lab = np.random.default_rng(8).integers(0, 20, (n, h, w), dtype=np.uint8)
    a = e.predict_mc(img, samples=3, keep_prob=0.5, sample_offset=2, argmax=False)
    b = e.predict_mc(img, samples=3, keep_prob=0.5, sample_offset=2, argmax=False)
    for u, v in zip(a, b):
        assert same_bits(u, v)
    c = e.predict_mc(img, samples=3, keep_prob=0.5, sample_offset=3, argmax=False)
    assert not same_bits(a[0], c[0])
    # device in, device out: the same bits
    import torch
    d = e.predict_mc(torch.from_numpy(img).cuda(), samples=3, keep_prob=0.5, sample_offset=2, argmax=False)
    for u, v in zip(a, d):
        assert v.is_cuda and same_bits(u, v.cpu().numpy())
    # training after a Monte-Carlo call: the masks and the loss of a fresh engine at the same step
    s6, s7 = (n, h // 32, w // 32, widths[5]), (n, h // 32, w // 32, widths[6])
    loss = e.forward_backward(img, lab, keep_prob=0.5)
    t6, t7 = e.dropout_masks(s6, s7)
    fresh = engine(precision, "small", tg, options={"deterministic": 1})
    loss_f = fresh.forward_backward(img, lab, keep_prob=0.5)
    f6, f7 = fresh.dropout_masks(s6, s7)
    assert same_bits(t6, f6) and same_bits(t7, f7) and loss == loss_f
    # ... and those are not a Monte-Carlo sample's masks
    e.predict_mc(img, samples=1, keep_prob=0.5, sample_offset=0)
    q6, _ = e.dropout_masks(s6, s7)
    assert not np.array_equal(q6, t6)
    e.close(); fresh.close()


# ---- e. the trunk runs once ----------------------------------------------------------------------------------------------------------
def _counts(e, call):
    e.profile(2); e.profile_reset()
    call()
    prof = e.profile_results()
    e.profile(0)
    return {k: int(v["launches"]) for k, v in prof.items() if not k.startswith("kernel:")}


def _is_fc(k):
    return "fc6" in k or "fc7" in k


def _is_trunk(k):
    return (k.startswith("conv") or k.startswith("wino_gemm_fwd") or k.startswith("maxpool") or k.startswith("derived:") or
            k in ("preprocess", "bf16_convert")) and not _is_fc(k)


@pytest.mark.parametrize("precision,ws,n,h,w", [("fp32", "small", 2, 64, 96), ("fp32", "small", 1, 128, 128), ("bf16_train", "small", 2, 64, 96), ("fp32", "full", 1, 32, 64)])
def test_the_trunk_runs_once_per_call(precision, ws, n, h, w):
    e = engine(precision, ws)
    img = images(n, h, w)
    e.predict(img); e.predict_mc(img, samples=4, keep_prob=0.5)          # (workspace and banks exist from here on)
    one = _counts(e, lambda: e.predict(img))
    mc4 = _counts(e, lambda: e.predict_mc(img, samples=4, keep_prob=0.5))
    print("predict: %s\npredict_mc, 4 samples: %s" % (one, mc4))
    trunk = [k for k in one if _is_trunk(k)]
    # (a pool is a launch of its own, "maxpool_fwd", or comes out of its block's last Winograd output transform, counted in "wino_transform" below)
    assert any(k.startswith("conv") for k in trunk) and any(k.startswith("derived:") for k in trunk)
    assert any(k.startswith("maxpool") for k in trunk) or "wino_transform" in one
    for k in trunk:
        assert mc4.get(k, 0) == one[k], (k, one[k], mc4.get(k, 0))
    assert not [k for k in mc4 if _is_trunk(k) and k not in one]
    fc = [k for k in one if _is_fc(k) and not k.startswith("derived:")]
    assert any("fc6" in k for k in fc) and any("fc7" in k for k in fc)
    for k in fc:
        assert mc4.get(k, 0) == 4 * one[k], (k, one[k], mc4.get(k, 0))
    assert mc4["mc_accumulate"] == 4 and "mc_accumulate" not in one and "softmax_argmax" not in mc4
    # the decoder: two skip heads once, the fc7 head and the three transposed convolutions once per sample
    assert one["score1x1_fwd"] == 3 and mc4["score1x1_fwd"] == 2 + 4
    assert mc4["tconv_fwd"] == 4 * one["tconv_fwd"]
    # the transforms around fc6's transform-domain GEMM (shared group "wino_transform"): the trunk's once, fc6's two per sample
    if any(k.startswith("wino_gemm_fc6") for k in one):
        assert mc4["wino_transform"] == one["wino_transform"] + 3 * 2
    elif "wino_transform" in one:
        assert mc4["wino_transform"] == one["wino_transform"]
    e.close()


# ---- f. state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16_train", "bf16_fc", "bf16_fwd", "f32x3"])
def test_state_after_a_call(precision):
    from fcn8s_tensorflow_amd.engine import Engine
    widths = SMALL64 if precision in ("bf16_train",) else SMALL
    P = params(widths, 30.0)

    def make():
        x = Engine(20, widths=widths, device_id=0, seed=5, precision=precision); x.set_params(P); return x
    e, fresh = make(), make()
    img = images(1, 128, 128)
    want = fresh.predict(img, argmax=False)
    kw = dict(samples=3, keep_prob=0.5, sample_offset=1, argmax=False)
    first = e.predict_mc(img, **kw)
    assert first[2].max() > 0                                  # every precision is served, with dropout on
    n1 = e.get_option("workspace_allocations")
    again = e.predict_mc(img, **kw)
    assert e.get_option("workspace_allocations") == n1
    for u, v in zip(first, again):
        assert same_bits(u, v)
    assert e.get_option("frozen") == 0
    assert same_bits(e.predict(img, argmax=False), want)
    e.freeze()
    assert same_bits(e.predict(img, argmax=False), want)
    third = e.predict_mc(img, **kw)
    assert e.get_option("frozen") == 1
    for u, v in zip(first, third):
        assert same_bits(u, v)
    assert same_bits(e.predict(img, argmax=False), want)
    n2 = e.get_option("workspace_allocations")
    e.predict_mc(img, **kw); e.predict(img)
    assert e.get_option("workspace_allocations") == n2
    # only some outputs
    p, ent, mi = e.predict_mc(img, entropy=False, **kw)
    assert ent is None and same_bits(p, first[0]) and same_bits(mi, first[2])
    p, ent, mi = e.predict_mc(img, mutual_information=False, **kw)
    assert mi is None and same_bits(ent, first[1])
    e.close(); fresh.close()


def test_refusals_launch_nothing():
    import ctypes as C
    from fcn8s_tensorflow_amd.engine import Engine
    e = engine("fp32", "small")
    img = images(1, 64, 64)
    out = np.empty((1, 64, 64), np.int64)
    ip, op = img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    e.profile(2); e.profile_reset()

    def rc(samples=4, keep=0.5, off=0, outp=op, ent=None, mi=None):
        return L.lib.fcn8s_predict_mc(e.h, ip, L.IMG_U8, 1, 64, 64, samples, keep, off, 1, outp, ent, mi, L.HOST)
    for bad in (dict(samples=0), dict(samples=257), dict(keep=0.0), dict(keep=1.5), dict(keep=float("nan")), dict(off=-1), dict(off=(1 << 30) - 3),
                dict(outp=None)):
        assert rc(**bad) == L.ERR_BAD_ARG, bad
    e.profile_reset()
    for bad in (dict(samples=0), dict(keep_prob=0.0), dict(sample_offset=-1)):
        with pytest.raises(ValueError):
            e.predict_mc(img, **bad)
    assert not any(v["launches"] for v in e.profile_results().values())       # nothing was launched by any refusal
    e.profile(0)
    a = e.predict_mc(img, samples=2, keep_prob=0.5, sample_offset=(1 << 30) - 2)
    assert np.isfinite(a[1]).all()
    e.close()
    # fp8_infer: the state error, with the reason in the text
    f = Engine(20, widths=SMALL64, device_id=0, precision="fp8_infer")
    f.set_params(params(SMALL64, 30.0))
    f.calibrate_fp8(img)
    with pytest.raises(Exception, match="dropout epilogue"):
        f.predict_mc(img, samples=2)
    assert L.lib.fcn8s_predict_mc(f.h, ip, L.IMG_U8, 1, 64, 64, 2, 0.5, 0, 1, op, None, None, L.HOST) == L.ERR_STATE
    f.predict(img)                                                        # ... and the model still predicts
    f.close()
