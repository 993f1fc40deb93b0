"""FCN8s.train(entropy_weight=...) on the GPU, on N = 2 labelled (+ M = 2 unlabelled) images of 64 x 96: two updates equal the same updates
driven by hand through Engine -- predict -> pseudo_label -> class_mix -> concatenate -> set_entropy_term(first_image = N) -> train_step with
`entropy_images='unlabeled'`; set_entropy_term -> train_step without a generator ('valid' pixels, a negative weight); both under
accumulation_steps = 2 -- bit for bit in every parameter; `entropy_loss` in scalars.jsonl equals Engine.entropy_term(); the engine's previous
setting is back after a normal return and after an exception from the generator; each refusal raises; and with entropy_weight = 0 nothing new is
launched or allocated."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_class_mix_facade_gpu import LR, N, SEED, THR, batches, gen, model, params_of, same_bits, unlabeled  # noqa: E402

WEIGHT = 0.1


def by_hand(b, items, uitems, A, weight, pixels, images):
    """The updates driven through Engine; returns Engine.entropy_term() after every update (the last micro-batch's)."""
    e = b.engine
    terms = []
    if uitems is None:
        e.set_entropy_term(weight, pixels)
    for u in range(2):
        for k in range(A):
            img, lab = items[u * A + k]
            X, Y = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
            if uitems is not None:
                uu = torch.from_numpy(uitems[u * A + k]).cuda()
                prob = b.predict(uu, argmax=False)
                pseudo, _ = e.pseudo_label(prob, thresholds=THR, ignore_id=255)
                uu, pseudo = e.class_mix(uu, pseudo, seed=SEED, draw=u * A + k)
                X, Y = torch.cat([X, uu]), torch.cat([Y, pseudo])
                e.set_entropy_term(weight, pixels, first_image=N if images == 'unlabeled' else 0)
            if k < A - 1:
                e.accumulate_step(X, Y, keep_prob=1.0, l2_rate=0.0)
            else:
                e.train_step(X, Y, LR, keep_prob=1.0, l2_rate=0.0)
        terms.append(e.entropy_term())
    return terms


MODES = {
    "unlabeled_images": dict(gen=True, A=1, weight=WEIGHT, pixels='unlabeled', images='unlabeled'),
    "unlabeled_images_accumulate": dict(gen=True, A=2, weight=WEIGHT, pixels='unlabeled', images='unlabeled'),
    "all_images_with_generator": dict(gen=True, A=1, weight=WEIGHT, pixels='all', images='all'),
    "no_generator_confidence_penalty": dict(gen=False, A=1, weight=-0.05, pixels='valid', images='all'),
    "no_generator_accumulate": dict(gen=False, A=2, weight=-0.05, pixels='valid', images='all'),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_train_with_the_entropy_term_equals_the_updates_driven_by_hand(mode, tmp_path):
    cfg = MODES[mode]
    A = cfg["A"]
    items = batches(2 * A)
    uitems = unlabeled(2 * A) if cfg["gen"] else None
    a = model()
    before = params_of(a)
    kw = dict(unlabeled_generator=gen(uitems), unlabeled_thresholds=THR, unlabeled_seed=SEED) if cfg["gen"] else {}
    if A > 1:
        kw.update(accumulation_steps=A)
    a.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, summaries_dir=str(tmp_path),
            summaries_frequency=1, entropy_weight=cfg["weight"], entropy_pixels=cfg["pixels"], entropy_images=cfg["images"], **kw)
    assert a.g_step == 2 and np.isfinite(a.training_loss) and a.engine.entropy_config is None
    got = params_of(a)
    assert any(np.abs(got[k] - before[k]).max() > 0 for k in got)
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path), 'training', 'scalars.jsonl'))]
    a.close()

    b = model()
    terms = by_hand(b, items, uitems, A, cfg["weight"], cfg["pixels"], cfg["images"])
    want = params_of(b)
    b.close()
    same_bits(got, want)
    assert [r["entropy_loss"] for r in rows] == terms and all(0.0 < t <= 1.0 for t in terms), (rows, terms)

    c = model()                                                                 # and the term has force: without it the parameters differ
    c.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
            **(dict(kw, unlabeled_generator=gen(uitems)) if cfg["gen"] else kw))
    off = params_of(c)
    c.close()
    assert any(np.abs(got[k] - off[k]).max() > 0 for k in got)


def test_the_previous_setting_is_restored_after_a_return_and_after_an_exception():
    m = model()
    m.engine.set_entropy_term(-0.25, 'valid', first_image=1)                    # a setting of the caller's own
    mine = dict(m.engine.entropy_config)
    assert mine == dict(weight=-0.25, pixels='valid', first_image=1)
    run = lambda items, **kw: m.train(gen(items), epochs=1, steps_per_epoch=len(items), learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                                      record_summaries=False, **kw)
    run(batches(1), entropy_weight=WEIGHT, entropy_pixels='all')
    assert m.engine.entropy_config == mine
    run(batches(1), unlabeled_generator=gen(unlabeled(1)), unlabeled_thresholds=THR, entropy_weight=WEIGHT, entropy_images='unlabeled')
    assert m.engine.entropy_config == mine
    with pytest.raises(RuntimeError, match="the generator broke"):
        run(batches(3), unlabeled_generator=gen(unlabeled(3), fail_after=1), unlabeled_thresholds=THR, entropy_weight=WEIGHT, entropy_images='unlabeled')
    assert m.engine.entropy_config == mine
    with pytest.raises(RuntimeError, match="the generator broke"):
        m.train(gen(batches(3), fail_after=1), epochs=1, steps_per_epoch=3, learning_rate_schedule=lambda s: LR, record_summaries=False,
                entropy_weight=WEIGHT)
    assert m.engine.entropy_config == mine
    run(batches(1))                                                             # entropy_weight = 0 leaves the caller's setting on
    assert m.engine.entropy_config == mine and m.engine.entropy_term() > 0
    m.engine.set_entropy_term()
    assert m.engine.entropy_config is None
    m.close()


def test_each_refusal():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    for kw in (dict(entropy_weight=float("nan")), dict(entropy_weight=float("inf")), dict(entropy_weight="much"), dict(entropy_weight=True),
               dict(entropy_weight=0.1, entropy_pixels='labeled'), dict(entropy_weight=0.1, entropy_images='some'),
               dict(entropy_weight=0.1, entropy_images='unlabeled'),             # no unlabeled_generator
               dict(entropy_weight=0.0, entropy_images='unlabeled'),             # ... whatever the weight
               dict(entropy_weight=0.0, entropy_pixels='none')):
        with pytest.raises(ValueError):
            run(**kw)
    assert m.engine.global_step == 0 and m.engine.entropy_config is None
    for kw in (dict(weight=float("nan")), dict(weight=1.0, pixels='x'), dict(weight=1.0, first_image=-1)):
        with pytest.raises(ValueError):
            m.engine.set_entropy_term(**kw)
    m.close()


def test_it_combines_with_a_teacher():
    T = model(seed=5)
    m = model()
    m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
            teacher=T, distill_weight=0.5, entropy_weight=WEIGHT, entropy_pixels='all')
    assert m.g_step == 1 and np.isfinite(m.training_loss) and m.engine.entropy_config is None and m.engine.soft_target_config is None
    T.close(); m.close()


def test_with_weight_zero_nothing_new_is_launched_or_allocated():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    run()
    m.engine.profile(True); m.engine.profile_reset()
    run()
    plain = {k: v["launches"] for k, v in m.engine.profile_results().items()}
    allocs = m.engine.get_option("workspace_allocations")
    m.engine.profile_reset()
    run(entropy_weight=0.0, entropy_pixels='all')
    assert {k: v["launches"] for k, v in m.engine.profile_results().items()} == plain and "entropy_term" not in plain
    assert m.engine.get_option("workspace_allocations") == allocs
    m.engine.profile_reset()
    run(entropy_weight=WEIGHT, entropy_pixels='all')
    assert m.engine.profile_results()["entropy_term"]["launches"] == 1 and m.engine.get_option("workspace_allocations") == allocs + 1
    m.close()
