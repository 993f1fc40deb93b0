"""Gradient accumulation over micro-batches, the global-norm clip and the non-finite guard at the model level (fcn8s_accumulate_bucket,
fcn8s_set_grad_clip, Engine.accumulate_step / set_grad_clip, FCN8s.train(accumulation_steps=, clip_global_norm=)).

Reference: NumPy float32 for the accumulated sum (bit for bit), optim.py's restatement for the clip's numbers, the library's own
optimizer ops at the reported scale for the clipped update, and -- for "micro-batches are the big batch" -- one process stepping on the
whole batch, to the bar tests/test_fake_rccl_gpu.py::test_two_native_ranks_step_equals_big_batch_step holds the two-rank split to."""
import ctypes as C
import json
import os
from glob import glob

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only: the synthetic parameters of the other GPU tests)
from fcn8s_tensorflow_amd import optim  # noqa: E402

SMALL = (8, 16, 32, 64, 64, 128, 128)


def _L():
    from fcn8s_tensorflow_amd import _lib
    return _lib


def engine(seed=7, **kw):
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=SMALL, seed=seed, **kw)
    e.set_params(orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05))
    return e


def batch(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 20, (n, h, w), dtype=np.uint8)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(b)))


def raw_forward_backward(e, img, lab, keep_prob=1.0, l2_rate=0.0, buckets=None):
    """fcn8s_forward_loss + the first `buckets` fcn8s_backward_bucket calls (all by default), nothing else"""
    L = _L()
    e._sync_stream()
    ka, pi, dt, pl, where, nhw = e._inputs(img, lab)
    N, H, W = (int(x) for x in nhw)
    L.check(L.lib.fcn8s_forward_loss(e.h, pi, dt, pl, N, H, W, keep_prob, l2_rate, where), e.h)
    for b in range(e.num_buckets if buckets is None else buckets):
        L.check(L.lib.fcn8s_backward_bucket(e.h, b), e.h)
    return ka


def test_the_sum_is_the_sum():
    """Three micro-batches of different shapes: after fold, fold, flush every gradient tensor is fl(fl(g1 + g2) + g3), bit for bit, and only the
    first fold allocates."""
    L = _L()
    e = engine()
    micro = [batch(2, 32, 64, 1), batch(1, 64, 64, 2), batch(2, 32, 64, 3)]
    gs, allocs = [], []
    for i, (img, lab) in enumerate(micro):
        raw_forward_backward(e, img, lab, l2_rate=1e-3)
        gs.append(e.get_grads())
        before = e.get_option("workspace_allocations")
        for b in range(e.num_buckets):
            L.check(L.lib.fcn8s_accumulate_bucket(e.h, b, 1 if i == 2 else 0), e.h)
        allocs.append(e.get_option("workspace_allocations") - before)
        assert e.pending_micro_batches == (0 if i == 2 else i + 1)
        if i < 2:                                                        # a fold leaves g alone
            for k, v in e.get_grads().items():
                assert np.array_equal(v, gs[i][k]), k
    assert allocs == [1, 0, 0]
    got = e.get_grads()
    for k in got:
        want = optim.accumulate([g[k] for g in gs])
        assert np.array_equal(got[k], want), k
    assert any(np.abs(got[k]).max() > 0 for k in got)
    # a flush with nothing pending launches nothing and changes nothing
    raw_forward_backward(e, *micro[0])
    g = e.get_grads()
    e.profile(2); e.profile_reset()
    for b in range(e.num_buckets):
        L.check(L.lib.fcn8s_accumulate_bucket(e.h, b, 1), e.h)
    assert "grad_accumulate" not in e.profile_results()
    e.profile(False)
    for k, v in e.get_grads().items():
        assert np.array_equal(v, g[k])
    e.close()


def _big_batch_reference(img, lab, clip=None):
    """two SGD-momentum steps of one process on all images -> (parameters before, after)"""
    L = _L()
    e = engine()
    if clip:
        e.set_grad_clip(clip)
    before = e.flat_params.cpu().numpy().copy()
    for _ in range(2):
        e.train_step(img, lab, 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
    after = e.flat_params.cpu().numpy().copy()
    e.close()
    return before, after


def test_micro_batches_are_the_big_batch():
    """The inputs and the bar of test_fake_rccl_gpu.py::test_two_native_ranks_step_equals_big_batch_step: two updates of 2 + 2 images against
    two steps on all 4 (SGD-momentum, keep_prob 1, l2 1e-3): update difference <= 2e-3 of the largest update entry."""
    L = _L()
    from tests.test_facade_gpu import gen
    img, lab = next(gen(4, 32, 64, 4, onehot=False))
    before, ref = _big_batch_reference(img, lab)
    e = engine()
    for i in range(2):
        e.accumulate_step(img[:2], lab[:2], keep_prob=1.0, l2_rate=1e-3)
        assert e.pending_micro_batches == 1 and e.global_step == i
        _, step = e.train_step(img[2:], lab[2:], 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        assert step == i + 1 and e.pending_micro_batches == 0
    got = e.flat_params.cpu().numpy()
    e.close()
    upd_ref, upd = ref - before, got - before
    assert np.abs(upd_ref).max() > 0
    err = np.abs(upd - upd_ref).max() / np.abs(upd_ref).max()
    print("accumulated vs big batch, two SGD updates: %.3g of the largest update entry" % err)
    assert err <= 2e-3, err


def test_fused_train_step_flushes_and_scales():
    """The same through the fused fcn8s_train_step after one accumulate_step (TF-Adam: compared with the split-phase route of Engine.train_step, which
    must give the same bits -- same kernels, same scale --, and the gradients it leaves with the big batch's to the same 2e-3 bar)."""
    L = _L()
    from tests.test_facade_gpu import gen
    img, lab = next(gen(4, 32, 64, 4, onehot=False))
    outs, grads = [], []
    for fused in (True, False):
        e = engine(options={"deterministic": 1})
        e.accumulate_step(img[:2], lab[:2], keep_prob=1.0, l2_rate=1e-3)
        if fused:
            e._sync_stream()
            ka, pi, dt, pl, where, nhw = e._inputs(img[2:], lab[2:])
            st = C.c_int64(0); lo = C.c_float(0)
            L.check(L.lib.fcn8s_train_step(e.h, pi, dt, pl, 2, 32, 64, 1e-3, 1.0, 1e-3, where, C.byref(lo), C.byref(st)), e.h)
            assert st.value == 1 and np.isfinite(lo.value)
        else:
            e.train_step(img[2:], lab[2:], 1e-3, keep_prob=1.0, l2_rate=1e-3)
        assert e.pending_micro_batches == 0 and e.global_step == 1
        outs.append(e.flat_params.cpu().numpy().copy()); grads.append(e.flat_grads.cpu().numpy().copy())
        e.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(grads[0], grads[1])
    # the flushed gradient is the sum of the two halves' = 2 x the big batch's mean gradient
    e = engine(options={"deterministic": 1})
    e.forward_backward(img, lab, keep_prob=1.0, l2_rate=1e-3)
    big = e.flat_grads.cpu().numpy().copy()
    e.close()
    err = np.abs(0.5 * grads[0] - big).max() / np.abs(big).max()
    print("fused flush: half the accumulated gradient vs the big batch's: %.3g of the largest entry" % err)
    assert err <= 2e-3, err


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_the_clip(opt):
    """max_norm = half the gradient's norm: update_stats() matches the restatement to the op-level bars (norm 4 ulps; c, s 2 ulps at the device's norm), and
    theta, m, v equal the existing op applied to copies with gs = stats.scale, bit for bit."""
    L = _L()
    e = engine()
    img, lab = batch(2, 32, 64, 5)
    e.forward_backward(img, lab, keep_prob=1.0, l2_rate=1e-3)
    g = e.flat_grads.cpu().numpy().copy()
    gs = 0.5
    norm = optim.global_norm(g, gs)
    assert norm > 0
    max_norm = float(norm) * 0.5
    e.set_grad_clip(max_norm)
    assert e.grad_clip == float(np.float32(max_norm))
    n = g.size
    th, m, v = (torch.from_numpy(a.copy()).cuda() for a in (e.flat_params.cpu().numpy(), np.zeros(n, np.float32), np.zeros(n, np.float32)))
    with pytest.raises(L.Fcn8sError):                                  # no clipped update yet
        e.update_stats()
    e.apply_update(1e-3, optimizer=L.OPT_TF_ADAM if opt == "adam" else L.OPT_SGD_MOMENTUM, grad_scale=gs)
    st = e.update_stats()
    assert e.global_step == 1 and st["skipped"] == 0
    print("clip[%s]: norm %r (restated %r, %.2f ulps), c %r, s %r" % (opt, st["norm"], norm, ulps(st["norm"], norm), st["clip_coef"], st["scale"]))
    assert ulps(st["norm"], norm) <= 4
    cw, sw, ok = optim.clip_scale(np.float32(st["norm"]), gs, max_norm)
    assert ok and ulps(st["clip_coef"], cw) <= 2 and ulps(st["scale"], sw) <= 2
    assert abs(st["clip_coef"] - 0.5) < 1e-5 and abs(st["scale"] - 0.25) < 1e-5
    gd = torch.from_numpy(g).cuda()
    if opt == "adam":
        L.check(L.lib.fcn8s_op_tf_adam(None, ptr(th), ptr(gd), ptr(m), ptr(v), n, 1, 1e-3, 0.9, 0.999, 1e-8, st["scale"]))
    else:
        L.check(L.lib.fcn8s_op_sgd_momentum(None, ptr(th), ptr(gd), ptr(m), n, 1e-3, 0.9, st["scale"]))
    torch.cuda.synchronize()
    mm, vv = e.get_opt_state()
    assert np.array_equal(e.flat_params.cpu().numpy(), th.cpu().numpy())
    assert np.array_equal(mm, m.cpu().numpy())
    if opt == "adam":
        assert np.array_equal(vv, v.cpu().numpy())
    assert np.array_equal(e.flat_grads.cpu().numpy(), g)              # the gradient buffer itself is not scaled
    # the setting survives a precision switch, an option and freezing; 0 / None switch it off
    e.set_precision('f32x3'); e.set_precision('fp32'); e.set_option("deterministic", 1); e.freeze(True); e.freeze(False)
    e.forward_backward(img, lab, keep_prob=1.0)
    e.apply_update(1e-3, grad_scale=1.0)
    assert e.update_stats()["clip_coef"] < 1.0
    e.set_grad_clip(None)
    assert e.grad_clip is None
    e.forward_backward(img, lab, keep_prob=1.0)
    e.apply_update(1e-3)
    with pytest.raises(L.Fcn8sError):
        e.update_stats()
    e.close()


def test_guard_only_changes_no_bit():
    """deterministic = 1, two fresh engines, three TF-Adam steps: clip off against max_norm = inf -- bit-identical parameters."""
    outs = []
    for clip in (None, float("inf")):
        e = engine(options={"deterministic": 1})
        e.set_grad_clip(clip)
        for i in range(3):
            img, lab = batch(2, 32, 64, 20 + i)
            _, step = e.train_step(img, lab, 1e-3, keep_prob=0.5, l2_rate=1e-4)
        assert step == 3
        if clip:
            st = e.update_stats()
            assert st["clip_coef"] == 1.0 and st["scale"] == 1.0 and st["skipped"] == 0 and np.isfinite(st["norm"]) and st["norm"] > 0
        outs.append((e.flat_params.cpu().numpy().copy(),) + e.get_opt_state())
        e.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_the_guard_skips_a_non_finite_update(bad):
    e = engine()
    e.set_grad_clip(1.0)
    img, lab = batch(2, 32, 64, 6)
    e.train_step(img, lab, 1e-3, keep_prob=1.0)                          # a clean step first: m and v exist and are not zero
    assert e.update_stats()["skipped"] == 0
    th0 = e.flat_params.cpu().numpy().copy(); m0, v0 = e.get_opt_state()
    e.forward_backward(img, lab, keep_prob=1.0)
    e.grad_view('fc6/weights').view(-1)[12345 % e.grad_view('fc6/weights').numel()] = bad
    e.apply_update(1e-3)
    st = e.update_stats()
    assert e.global_step == 2 and st["skipped"] == 1 and not np.isfinite(st["norm"])
    m1, v1 = e.get_opt_state()
    assert e.flat_params.cpu().numpy().tobytes() == th0.tobytes() and m1.tobytes() == m0.tobytes() and v1.tobytes() == v0.tobytes()
    e.train_step(img, lab, 1e-3, keep_prob=1.0)                          # a clean step updates again; the counter stays
    st = e.update_stats()
    assert e.global_step == 3 and st["skipped"] == 1 and np.isfinite(st["norm"])
    assert not np.array_equal(e.flat_params.cpu().numpy(), th0)
    e.close()


def test_defaults_launch_nothing_new():
    """A = 1 and no clip: a train_step's detailed profile has neither new group, and the model allocates what a model that never heard of the feature
    allocates (an engine that used the feature once and switched it off again, against a fresh one)."""
    img, lab = batch(2, 32, 64, 7)
    plain = engine()
    plain.train_step(img, lab, 1e-3, keep_prob=1.0)
    plain_allocs = plain.get_option("workspace_allocations")
    plain.profile(2); plain.profile_reset()
    plain.train_step(img, lab, 1e-3, keep_prob=1.0)
    groups = plain.profile_results()
    assert "adam" in groups and "grad_accumulate" not in groups and "grad_norm" not in groups
    assert plain.get_option("workspace_allocations") == plain_allocs
    plain.close()
    # the groups are there when the feature is on ...
    e = engine()
    e.set_grad_clip(float("inf"))
    e.profile(2)
    e.accumulate_step(img, lab, keep_prob=1.0)
    e.train_step(img, lab, 1e-3, keep_prob=1.0)
    groups = e.profile_results()
    nb = e.num_buckets
    assert groups["grad_accumulate"]["launches"] == 2 * nb and groups["grad_norm"]["launches"] == 1
    total = e.flat_grads.numel()
    assert groups["grad_accumulate"]["bytes"] == (8 + 12) * total and groups["grad_norm"]["bytes"] == 4 * total
    assert e.get_option("workspace_allocations") == plain_allocs + 1          # the accumulator, once
    # ... and gone again with the defaults
    e.set_grad_clip(None)
    e.profile_reset()
    e.train_step(img, lab, 1e-3, keep_prob=1.0)
    groups = e.profile_results()
    assert groups["grad_accumulate"]["launches"] == 0 and groups["grad_norm"]["launches"] == 0
    assert e.get_option("workspace_allocations") == plain_allocs + 1
    e.close()


def test_errors():
    L = _L()
    img, lab = batch(2, 32, 64, 8)
    e = engine(options={"deterministic": 1})
    # folding before backward; a bad bucket
    assert L.lib.fcn8s_accumulate_bucket(e.h, 0, 0) == L.ERR_STATE
    assert L.lib.fcn8s_accumulate_bucket(e.h, e.num_buckets, 0) == L.ERR_BAD_ARG
    raw_forward_backward(e, img, lab, buckets=1)
    assert L.lib.fcn8s_accumulate_bucket(e.h, 1, 0) == L.ERR_STATE          # bucket 1's backward call has not run
    assert L.lib.fcn8s_accumulate_bucket(e.h, 0, 0) == L.OK
    assert L.lib.fcn8s_accumulate_bucket(e.h, 0, 0) == L.ERR_STATE          # a double fold
    assert L.lib.fcn8s_accumulate_bucket(e.h, 0, 1) == L.ERR_STATE          # ... or a flush of what was just folded
    for b in range(1, e.num_buckets):
        L.check(L.lib.fcn8s_backward_bucket(e.h, b), e.h)
        L.check(L.lib.fcn8s_accumulate_bucket(e.h, b, 0), e.h)
    assert e.pending_micro_batches == 1
    # a forgotten flush: the update is refused, parameters and step untouched
    th0 = e.flat_params.cpu().numpy().copy()
    with pytest.raises(L.Fcn8sError, match="not flushed"):
        e.apply_update(1e-3)
    assert L.lib.fcn8s_apply_update(e.h, L.OPT_TF_ADAM, 1e-3, 1.0) == L.ERR_STATE
    assert e.global_step == 0 and np.array_equal(e.flat_params.cpu().numpy(), th0)
    # after the next forward pass the old backward pass's buckets cannot be folded again
    e._sync_stream()
    ka, pi, dt, pl, where, nhw = e._inputs(img, lab)
    L.check(L.lib.fcn8s_forward_loss(e.h, pi, dt, pl, 2, 32, 64, 1.0, 0.0, where), e.h)
    assert L.lib.fcn8s_accumulate_bucket(e.h, 0, 0) == L.ERR_STATE
    # discard: the next plain step equals a plain step
    e.discard_accumulated()
    assert e.pending_micro_batches == 0
    _, step = e.train_step(img, lab, 1e-3, keep_prob=1.0)
    ref = engine(options={"deterministic": 1})
    ref.train_step(img, lab, 1e-3, keep_prob=1.0)
    assert step == 1 and np.array_equal(e.flat_params.cpu().numpy(), ref.flat_params.cpu().numpy())
    ref.close()
    # a bad max_norm
    for bad in (-1.0, float("nan"), -float("inf")):
        assert L.lib.fcn8s_set_grad_clip(e.h, bad) == L.ERR_BAD_ARG
        with pytest.raises(ValueError):
            e.set_grad_clip(bad)
    assert e.grad_clip is None
    assert L.lib.fcn8s_get_update_stats(e.h, None, None, None, None) == L.ERR_STATE
    e.close()
    # fp8_infer refuses the new training call as it refuses the others (the mode needs channel widths that are multiples of 64)
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(20, widths=(64,) * 7, seed=7)
    e.init_params(0)
    raw_forward_backward(e, img, lab)
    e.set_precision('fp8_infer')
    assert L.lib.fcn8s_accumulate_bucket(e.h, 0, 0) == L.ERR_STATE
    assert b"fp8" in L.lib.fcn8s_last_error(e.h).lower()
    with pytest.raises(L.Fcn8sError):
        e.accumulate_step(img, lab)
    e.close()


def _gen_counting(count, n=2, h=32, w=64, seed=0, fail_at=None):
    rng = np.random.default_rng(seed)
    while True:
        if fail_at is not None and count[0] >= fail_at:
            raise RuntimeError("the generator gave up")
        count[0] += 1
        img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        lab = rng.integers(0, 20, (n, h, w), dtype=np.uint8)
        yield img, orc.one_hot(lab, 20)


def test_facade_train_accumulates_and_clips(tmp_path):
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    from fcn8s_tensorflow_amd import tf_events
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=SMALL)
    for kw in (dict(accumulation_steps=0), dict(accumulation_steps=1.5), dict(clip_global_norm=0.0), dict(clip_global_norm=-1.0),
               dict(clip_global_norm=float("nan"))):
        with pytest.raises(ValueError):
            m.train(_gen_counting([0]), 1, 1, lambda s: 1e-3, **kw)
    count = [0]
    lrs = []
    m.train(_gen_counting(count), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: lrs.append(s) or 1e-3, accumulation_steps=2,
            clip_global_norm=1.0, summaries_dir=str(tmp_path / 'tb'), summaries_name='run', summaries_frequency=1)
    assert count[0] == 4 and m.g_step == 2 and m.engine.global_step == 2 and lrs == [0, 1, 2]
    assert np.isfinite(m.training_loss) and m.engine.grad_clip is None and m.engine.pending_micro_batches == 0
    recs = [json.loads(l) for l in open(tmp_path / 'tb' / 'run' / 'scalars.jsonl')]
    assert [r["step"] for r in recs] == [1, 2]
    for r in recs:
        assert {"total_loss", "learning_rate", "grad_norm", "clip_coef"} <= set(r)
        assert r["grad_norm"] > 0 and 0 < r["clip_coef"] <= 1.0
        assert abs(r["clip_coef"] - min(1.0, 1.0 / r["grad_norm"])) < 1e-5
    (tr,) = glob(str(tmp_path / 'tb' / 'run' / 'events.out.tfevents.*'))
    evs = tf_events.read_events(tr)
    assert {"total_loss", "learning_rate", "grad_norm", "clip_coef"} <= set(evs[1]['scalars'])
    # without a clip the two scalars are not recorded
    m.train(_gen_counting([0]), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: 1e-3, summaries_dir=str(tmp_path / 'tb'),
            summaries_name='plain', summaries_frequency=1)
    (rec,) = [json.loads(l) for l in open(tmp_path / 'tb' / 'plain' / 'scalars.jsonl')]
    assert "grad_norm" not in rec and "clip_coef" not in rec and rec["step"] == 3
    # a generator that raises in the middle of an update: the clip is back to what it was, nothing stays pending
    m.engine.set_grad_clip(5.0)
    with pytest.raises(RuntimeError, match="gave up"):
        m.train(_gen_counting([0], fail_at=3), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: 1e-3, accumulation_steps=2,
                clip_global_norm=float("inf"), record_summaries=False)
    assert m.engine.grad_clip == 5.0 and m.engine.pending_micro_batches == 0
    m.close()
