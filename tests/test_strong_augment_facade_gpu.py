"""FCN8s.train(unlabeled_generator=..., unlabeled_augment=...) on the GPU: two updates of a narrow model on N = 2 labelled and M = 2 unlabelled
images of 64 x 96 equal the same updates driven by hand through Engine (predict -> pseudo_label -> class_mix -> strong_augment -> concatenate ->
train_step), bit for bit in every parameter -- labelled by the student itself and by another model, with accumulation_steps = 2 and without
mixing; the labeler is given the clean batch; each refusal raises; and with `unlabeled_augment=None` nothing new is launched or allocated."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import strong_augment as SA  # noqa: E402
from tests.test_class_mix_facade_gpu import LR, M, H, W, SEED, THR, batches, gen, model, params_of, same_bits, unlabeled  # noqa: E402

# every image is recoloured (so the student's input differs from the labeler's in every pixel row) and half of them are blurred
AUG = dict(jitter_p=1.0, blur_p=0.5)


def by_hand(b, items, uitems, aug, A=1, labeler=None, mix=True, updates=2):
    e = b.engine
    for u in range(updates):
        for k in range(A):
            img, lab = items[u * A + k]
            x, ids, uu = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(uitems[u * A + k]).cuda()
            prob = (labeler or b).predict(uu, argmax=False)
            pseudo, _ = e.pseudo_label(prob, thresholds=THR, ignore_id=255)
            if mix:
                uu, pseudo = e.class_mix(uu, pseudo, seed=SEED, draw=u * A + k)
            uu = e.strong_augment(uu, seed=SEED, draw=u * A + k, jitter=aug["jitter"], blur=aug["blur"])
            X, Y = torch.cat([x, uu]), torch.cat([ids, pseudo])
            if k < A - 1:
                e.accumulate_step(X, Y, keep_prob=1.0, l2_rate=0.0)
            else:
                e.train_step(X, Y, LR, keep_prob=1.0, l2_rate=0.0)


MODES = {
    "self": dict(),
    "model": dict(other=True),
    "accumulate": dict(A=2),
    "no_mix": dict(mix=False),
    "defaults": dict(augment=True),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_augmented_self_training_equals_the_updates_driven_by_hand(mode):
    cfg = MODES[mode]
    A, mix, augment = cfg.get("A", 1), cfg.get("mix", True), cfg.get("augment", AUG)
    other = model(seed=5) if cfg.get("other") else None
    items, uitems = batches(2 * A), unlabeled(2 * A)
    a = model()
    kw = dict(unlabeled_labeler=other) if other is not None else {}
    if A > 1:
        kw.update(accumulation_steps=A)
    a.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
            unlabeled_generator=gen(uitems), unlabeled_thresholds=THR, unlabeled_mix=mix, unlabeled_seed=SEED, unlabeled_augment=augment, **kw)
    assert a.g_step == 2 and np.isfinite(a.training_loss)
    got = params_of(a)
    a.close()

    aug = SA.validate(augment)
    b = model()
    by_hand(b, items, uitems, aug, A=A, labeler=other, mix=mix)
    want = params_of(b)
    b.close()
    same_bits(got, want)
    if other is not None:
        other.close()


def test_the_augmentation_changes_the_training_and_the_labeler_sees_the_clean_batch():
    items, uitems = batches(2), unlabeled(2)
    seen = []
    res = []
    for augment in (None, AUG):
        m = model()
        predict = m.predict

        def spy(images, *a, _predict=predict, **kw):
            if isinstance(images, torch.Tensor) and images.shape[0] == M and not kw.get("argmax", True):
                seen.append(images.cpu().numpy().copy())
            return _predict(images, *a, **kw)
        m.predict = spy
        m.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
                unlabeled_generator=gen(uitems), unlabeled_thresholds=THR, unlabeled_seed=SEED, unlabeled_augment=augment)
        res.append(params_of(m))
        m.close()
    assert len(seen) == 4 and all((s == u).all() for s, u in zip(seen, uitems + uitems))      # the clean images, with and without the augmentation
    assert any(np.abs(res[0][k] - res[1][k]).max() > 0 for k in res[0])
    aug = SA.validate(AUG)                                                                      # and the op did change what the student saw
    out, par = SA.augment_numpy(uitems[0], SEED, 0, aug["jitter"], aug["blur"])
    assert par[:, 0].all() and (out != uitems[0]).any()


def test_each_refusal():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    u = lambda: gen(unlabeled(1))
    for kw in (dict(unlabeled_augment=True), dict(unlabeled_augment=AUG), dict(unlabeled_augment={}),                      # no generator
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=1),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment="strong"),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(gamma=0.5)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(jitter_p=1.5)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(hue=-0.1)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(radius=8)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(levels=17)),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(sigma=(0.0, 1.0))),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(jitter_p=0, blur_p=0))):
        with pytest.raises(ValueError):
            run(**kw)
    assert not m.g_step and not m.engine.pending_micro_batches                                    # (every refusal comes before the first batch is drawn)
    run(unlabeled_generator=u(), unlabeled_thresholds=THR, unlabeled_augment=dict(blur_p=0))      # one stage alone is fine
    assert m.g_step == 1
    m.close()


def test_without_the_keyword_nothing_new_is_launched_or_allocated():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, unlabeled_generator=gen(unlabeled(1)), unlabeled_thresholds=THR, **kw)
    run()
    m.engine.profile(True); m.engine.profile_reset()
    a0 = m.engine.get_option("workspace_allocations")
    run()
    plain = {k: v["launches"] for k, v in m.engine.profile_results().items()}
    a1 = m.engine.get_option("workspace_allocations")        # ('self': the student's engine re-carves its workspace between predict and step)
    gc.collect(); mem = torch.cuda.memory_allocated()
    m.engine.profile_reset()
    run(unlabeled_augment=None)
    assert {k: v["launches"] for k, v in m.engine.profile_results().items()} == plain
    assert m.engine.get_option("workspace_allocations") - a1 == a1 - a0 and not hasattr(m.engine, "_strong_augment_work")
    gc.collect(); assert torch.cuda.memory_allocated() == mem
    run(unlabeled_augment=True)
    assert hasattr(m.engine, "_strong_augment_work")
    m.close()
