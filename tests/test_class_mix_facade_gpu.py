"""FCN8s.train(unlabeled_generator=...) on the GPU: two updates of a narrow model on N = 2 labelled and M = 2 unlabelled images of 64 x 96 equal
the same updates driven by hand through Engine (predict -> pseudo_label -> class_mix -> concatenate -> train_step), bit for bit in every
parameter -- labelled by the student itself, by another model and by the student's averaged weights (where the shadow is compared too), with
accumulation_steps = 2 and without mixing; `pseudo_kept` in scalars.jsonl equals the op's counts; the labeler's frozen state and the student's
raw weights hold after an exception; each refusal raises; and without a generator nothing new is launched or allocated."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NARROW = (8, 16, 32, 64, 64, 128, 128)
N, M, H, W = 2, 2, 64, 96
LR, SEED, EMA = 1e-3, 5, 0.9
THR = np.linspace(0.45, 0.75, 20).astype(np.float32)


def batches(count, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
        lab = rng.integers(0, 20, (N, H, W), dtype=np.uint8)
        lab[rng.random((N, H, W)) < 0.1] = 255
        out.append((img, lab))
    return out


def unlabeled(count, seed=100, m=M, h=H, w=W):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (m, h, w, 3), dtype=np.uint8) for _ in range(count)]


def gen(items, fail_after=None):
    for k, item in enumerate(items):
        if fail_after is not None and k == fail_after:
            raise RuntimeError("the generator broke")
        yield item


def model(seed=3, num_classes=20):
    """A narrow model with lively decoder weights (tests/test_temperature_facade_gpu.py: the median confidence is about 0.7), so that the
    thresholds keep some pixels of several classes and drop others."""
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    from oracle import fcn8s_oracle as orc
    m = FCN8s(vgg16_dir='synthetic:%d' % seed, num_classes=num_classes, widths=NARROW)
    m.engine.set_option("deterministic", 1)
    m.engine.set_params(orc.init_params(num_classes, NARROW, seed=seed, decoder_std_scale=12.0, bias_std=0.05))
    return m


def params_of(m):
    return {k: v.copy() for k, v in m.engine.get_params().items()}


def same_bits(got, want):
    for k in want:
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)


def by_hand(b, items, uitems, A=1, labeler=None, ema=False, mix=True, updates=2):
    """The updates driven through Engine; returns the kept share of every update's last micro-batch."""
    e = b.engine
    if ema:
        e.set_ema(EMA, True)
    kept = []
    for u in range(updates):
        for k in range(A):
            img, lab = items[u * A + k]
            x, ids, uu = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(uitems[u * A + k]).cuda()
            with (e.averaged_weights() if ema else contextlib.nullcontext()):
                prob = (labeler or b).predict(uu, argmax=False)
            pseudo, tables = e.pseudo_label(prob, thresholds=THR, ignore_id=255)
            if mix:
                uu, pseudo = e.class_mix(uu, pseudo, seed=SEED, draw=u * A + k)
            X, Y = torch.cat([x, uu]), torch.cat([ids, pseudo])
            if k < A - 1:
                e.accumulate_step(X, Y, keep_prob=1.0, l2_rate=0.0)
            else:
                e.train_step(X, Y, LR, keep_prob=1.0, l2_rate=0.0)
        kept.append(float(tables["counts"][:, 0].sum().item()) / (M * H * W))
    return kept


MODES = {
    "self": dict(),
    "model": dict(other=True),
    "ema": dict(ema=True),
    "accumulate": dict(A=2),
    "no_mix": dict(mix=False),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_self_training_equals_the_updates_driven_by_hand(mode, tmp_path):
    cfg = MODES[mode]
    A, ema, mix = cfg.get("A", 1), cfg.get("ema", False), cfg.get("mix", True)
    other = model(seed=5) if cfg.get("other") else None
    items, uitems = batches(2 * A), unlabeled(2 * A)
    a = model()
    before = params_of(a)
    kw = dict(unlabeled_labeler=other if other is not None else ('ema' if ema else 'self'))
    if ema:
        kw.update(ema_decay=EMA)
    if A > 1:
        kw.update(accumulation_steps=A)
    a.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, summaries_dir=str(tmp_path),
            summaries_frequency=1, unlabeled_generator=gen(uitems), unlabeled_thresholds=THR, unlabeled_mix=mix, unlabeled_seed=SEED, **kw)
    assert a.g_step == 2 and np.isfinite(a.training_loss)
    got = params_of(a)
    got_shadow = a.engine.get_ema() if ema else None
    assert any(np.abs(got[k] - before[k]).max() > 0 for k in got)
    assert not a.engine.ema_info()['swapped'] and a.engine.ema_config is None
    if other is not None:
        assert not other.engine.get_option("frozen")
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path), 'training', 'scalars.jsonl'))]
    a.close()

    b = model()
    kept = by_hand(b, items, uitems, A=A, labeler=other, ema=ema, mix=mix)
    want = params_of(b)
    if ema:
        np.testing.assert_array_equal(got_shadow.view(np.uint32), b.engine.get_ema().view(np.uint32))
    b.close()
    same_bits(got, want)
    assert [r["pseudo_kept"] for r in rows] == kept and all(0.0 < s < 1.0 for s in kept), (rows, kept)
    if other is not None:
        other.close()


def test_mixing_changes_the_training_and_one_hot_labels_train_as_ids_do():
    items, uitems = [(img, lab % 20) for img, lab in batches(2)], unlabeled(2)              # (an all-zero one-hot row is refused: no ignore labels here)
    onehot = [(img, np.eye(20, dtype=np.float32)[lab]) for img, lab in items]
    res = []
    for feed, mix in ((items, True), (items, False), (onehot, True)):
        m = model()
        m.train(gen(feed), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
                unlabeled_generator=gen([(u, None) for u in uitems]), unlabeled_thresholds=0.5, unlabeled_mix=mix)      # tuples: the first element
        res.append(params_of(m))
        m.close()
    same_bits(res[2], res[0])
    assert any(np.abs(res[0][k] - res[1][k]).max() > 0 for k in res[0])


@pytest.mark.parametrize("frozen", [False, True])
def test_the_labelers_frozen_state_and_the_raw_weights_hold_after_an_exception(frozen):
    other = model(seed=5)
    other.engine.freeze(frozen)
    m = model()
    run = lambda **kw: m.train(gen(batches(3)), epochs=1, steps_per_epoch=3, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, unlabeled_generator=gen(unlabeled(3), fail_after=1), unlabeled_thresholds=THR, **kw)
    with pytest.raises(RuntimeError, match="the generator broke"):
        run(unlabeled_labeler=other)
    assert bool(other.engine.get_option("frozen")) == frozen and m.g_step == 1
    with pytest.raises(RuntimeError, match="the generator broke"):
        run(unlabeled_labeler='ema', ema_decay=EMA)
    info = m.engine.ema_info()
    assert info['has_shadow'] and not info['swapped'] and m.engine.ema_config is None and m.g_step == 2
    raw = params_of(m)
    assert np.abs(m.engine.get_ema() - m.engine.flat_params.cpu().numpy()).max() > 0          # the live weights are not the average
    m.engine.train_step(*batches(1)[0], LR)                                                  # and training goes on (it raises while swapped)
    assert any(np.abs(params_of(m)[k] - raw[k]).max() > 0 for k in raw)
    other.close(); m.close()


def test_each_refusal():
    m, other19, other20 = model(), model(seed=5, num_classes=19), model(seed=5)
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    u = lambda **kw: gen(unlabeled(1, **kw))
    for kw in (dict(unlabeled_generator=u(), unlabeled_thresholds=THR, teacher=other20),                 # together with teacher=
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_labeler='ema'),        # no average
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_labeler=other19),      # another class count
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_labeler=m),            # the student as a frozen labeler
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_labeler='teacher'),
               dict(unlabeled_generator=u()),                                                           # no thresholds anywhere
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR[:19]),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_predict=dict(argmax=True)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_predict=dict(samples=2, flip=True)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_predict=dict(mi_max=0.1)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_mix=1),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_seed=-1),
               dict(unlabeled_generator=u(m=1), unlabeled_thresholds=THR),                              # M < 2
               dict(unlabeled_generator=u(h=32), unlabeled_thresholds=THR),                             # another size
               dict(unlabeled_thresholds=THR), dict(unlabeled_predict=dict(flip=True)), dict(unlabeled_labeler='ema')):      # no generator
        with pytest.raises(ValueError):
            run(**kw)
    assert m.g_step == 0 and not m.engine.pending_micro_batches
    m.pseudo_label_thresholds = THR                                                                     # None takes the model's
    run(unlabeled_generator=u(), unlabeled_predict=dict(scales=(1.0,), flip=True))
    assert m.g_step == 1
    other19.close(); other20.close(); m.close()


def test_without_a_generator_nothing_new_is_launched_or_allocated():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    run()
    m.engine.profile(True); m.engine.profile_reset()
    run()
    plain = {k: v["launches"] for k, v in m.engine.profile_results().items()}
    allocs = m.engine.get_option("workspace_allocations")
    m.engine.profile_reset()
    run(unlabeled_generator=None)
    assert {k: v["launches"] for k, v in m.engine.profile_results().items()} == plain
    assert m.engine.get_option("workspace_allocations") == allocs and not hasattr(m.engine, "_class_mix_work")
    m.close()
