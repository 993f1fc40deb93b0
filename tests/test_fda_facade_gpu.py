"""FCN8s.train(unlabeled_generator=..., fda_beta=...) on the GPU: two updates of a narrow model on N = 2 labelled and M = 2 unlabelled images of
64 x 96 equal the same updates driven by hand through Engine (fda_transfer -> predict -> pseudo_label -> class_mix -> concatenate -> train_step),
bit for bit in every parameter -- labelled by the student itself, with accumulation_steps = 2 and without mixing; the labeler is given the clean
batch and the adaptation the clean targets; `FCN8s.fda_transfer` on NumPy input equals `Engine.fda_transfer`; each refusal raises, a half-width above 96 when a batch shows its size; and with
`fda_beta=None` nothing new is launched or allocated."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import fda as FDA  # noqa: E402
from tests.test_class_mix_facade_gpu import LR, N, M, H, W, SEED, THR, batches, gen, model, params_of, same_bits, unlabeled  # noqa: E402

BETA = 0.05                                                      # b = floor(64 * 0.05) = 3


def by_hand(b, items, uitems, A=1, mix=True, updates=2):
    e = b.engine
    for u in range(updates):
        for k in range(A):
            img, lab = items[u * A + k]
            x, ids, uu = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(uitems[u * A + k]).cuda()
            draw = u * A + k
            x = e.fda_transfer(x, uu, beta=BETA, pair=[(n + draw) % M for n in range(N)])
            prob = b.predict(uu, argmax=False)
            pseudo, _ = e.pseudo_label(prob, thresholds=THR, ignore_id=255)
            if mix:
                uu, pseudo = e.class_mix(uu, pseudo, seed=SEED, draw=draw)
            X, Y = torch.cat([x, uu]), torch.cat([ids, pseudo])
            if k < A - 1:
                e.accumulate_step(X, Y, keep_prob=1.0, l2_rate=0.0)
            else:
                e.train_step(X, Y, LR, keep_prob=1.0, l2_rate=0.0)


MODES = {"self": dict(), "accumulate": dict(A=2), "no_mix": dict(mix=False)}


@pytest.mark.parametrize("mode", list(MODES))
def test_adapted_self_training_equals_the_updates_driven_by_hand(mode):
    cfg = MODES[mode]
    A, mix = cfg.get("A", 1), cfg.get("mix", True)
    items, uitems = batches(2 * A), unlabeled(2 * A)
    a = model()
    kw = dict(accumulation_steps=A) if A > 1 else {}
    a.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
            unlabeled_generator=gen(uitems), unlabeled_thresholds=THR, unlabeled_mix=mix, unlabeled_seed=SEED, fda_beta=BETA, **kw)
    assert a.g_step == 2 and np.isfinite(a.training_loss)
    got = params_of(a)
    a.close()
    b = model()
    by_hand(b, items, uitems, A=A, mix=mix)
    want = params_of(b)
    b.close()
    same_bits(got, want)


def test_the_adaptation_changes_the_training_and_the_labeler_and_the_op_see_the_clean_batch():
    assert FDA.half_width(H, W, BETA) == 3
    items, uitems = batches(2), unlabeled(2)
    seen, styles, res = [], [], []
    for beta in (None, BETA):
        m = model()
        predict, transfer = m.predict, m.engine.fda_transfer

        def spy(images, *a, _predict=predict, **kw):
            if isinstance(images, torch.Tensor) and images.shape[0] == M and not kw.get("argmax", True):
                seen.append(images.cpu().numpy().copy())
            return _predict(images, *a, **kw)

        def spy_fda(images, targets, *a, _transfer=transfer, **kw):
            styles.append((images.cpu().numpy().copy(), targets.cpu().numpy().copy(), kw["pair"].cpu().tolist(), kw["b"]))
            return _transfer(images, targets, *a, **kw)
        m.predict, m.engine.fda_transfer = spy, spy_fda
        m.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
                unlabeled_generator=gen(uitems), unlabeled_thresholds=THR, unlabeled_seed=SEED, fda_beta=beta)
        res.append(params_of(m))
        m.close()
    assert len(seen) == 4 and all((s == u).all() for s, u in zip(seen, uitems + uitems))      # the clean images, with and without the adaptation
    assert len(styles) == 2                                                                    # (None: the op is not called)
    for k, (x, t, pair, b) in enumerate(styles):
        assert (x == items[k][0]).all() and (t == uitems[k]).all() and pair == [(n + k) % M for n in range(N)] and b == 3
    assert any(np.abs(res[0][k] - res[1][k]).max() > 0 for k in res[0])
    assert (FDA.to_uint8(FDA.transfer_numpy(items[0][0], uitems[0], 3)) != items[0][0]).any()   # and the op does change what the student sees


def test_the_facade_on_numpy_input_equals_the_engine_on_device_tensors():
    m = model()
    img, trg = batches(1)[0][0], unlabeled(1)[0]
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(trg).cuda()
    for kw in (dict(), dict(beta=BETA), dict(beta=0.09, pair=[1, 1])):
        want = m.engine.fda_transfer(x, t, **kw).cpu().numpy()
        got = m.fda_transfer(img, trg, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and (got == want).all()
        dev = m.fda_transfer(x, t, **kw)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and (dev.cpu().numpy() == want).all()
    ref = FDA.transfer_numpy(img, trg, 3)                                                       # and it is the operation: within 0.5 + 8 E of float64
    E = np.abs(FDA.transfer_numpy(img, trg, 3, dtype=np.float32) - ref).max()
    bar = 8 * max(float(E), float(np.spacing(np.float32(256))))
    assert np.abs(m.fda_transfer(img, trg, beta=BETA).astype(np.float64) - np.clip(ref, 0, 255)).max() <= 0.5 + bar
    with pytest.raises(ValueError):
        m.fda_transfer(img.astype(np.float32), trg)
    with pytest.raises(ValueError):
        m.fda_transfer(img, trg[:, :32])
    m.close()


def test_each_refusal():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    u = lambda: gen(unlabeled(1))
    for kw in (dict(fda_beta=0.01), dict(fda_beta=0.09),                                       # no generator
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta=0.0),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta=-0.01),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta=0.1),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta="0.01"),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta=True),
               dict(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta=float("nan"))):
        with pytest.raises(ValueError):
            run(**kw)
    assert not m.g_step and not m.engine.pending_micro_batches                                  # (every refusal comes before the first batch is drawn)
    run(unlabeled_generator=u(), unlabeled_thresholds=THR, fda_beta=0.09)
    assert m.g_step == 1
    m.close()


@pytest.mark.parametrize("A", [1, 2], ids=["first_batch", "second_micro_batch"])
def test_a_half_width_above_96_is_refused_when_a_batch_shows_its_size(A):
    """floor(1080 * 0.09) = 97 > 96.  A generator does not tell its size before it yields, so the refusal comes in the step: before anything of that
    batch is launched and before the unlabelled batch is drawn.  With accumulation_steps = 2 the first micro-batch is small and goes through, the
    second is refused: the update it cuts short is discarded."""
    S = 1080
    assert FDA.half_width(S, S, 0.09) == 97 and FDA.half_width(1077, 2000, 0.09) == 96
    rng = np.random.default_rng(5)
    big = (rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8), rng.integers(0, 20, (N, S, S), dtype=np.uint8))
    ubig = rng.integers(0, 256, (M, S, S, 3), dtype=np.uint8)
    items, uitems = (batches(1) + [big], unlabeled(1) + [ubig]) if A == 2 else ([big], [ubig])
    m = model()
    before = params_of(m)
    drawn = gen(uitems)
    with pytest.raises(ValueError, match="half-width"):
        m.train(gen(items), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
                unlabeled_generator=drawn, unlabeled_thresholds=THR, unlabeled_seed=SEED, fda_beta=0.09, accumulation_steps=A)
    assert m.g_step == 0 and m.engine.global_step == 0 and not m.engine.pending_micro_batches
    assert hasattr(m.engine, "_fda_work") == (A == 2)                                           # (the small micro-batch ran the op, the refused batch nothing)
    assert next(drawn) is ubig                                                                  # the refused batch's unlabelled images were not drawn
    same_bits(params_of(m), before)                                                             # no update happened
    m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
            unlabeled_generator=gen(unlabeled(1)), unlabeled_thresholds=THR, unlabeled_seed=SEED, fda_beta=0.09)
    assert m.g_step == 1 and np.isfinite(m.training_loss) and not m.engine.pending_micro_batches   # and the model still trains
    want = model()
    want.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
               unlabeled_generator=gen(unlabeled(1)), unlabeled_thresholds=THR, unlabeled_seed=SEED, fda_beta=0.09)
    same_bits(params_of(m), params_of(want))                                                    # as one that never met the refusal
    m.close(); want.close()


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
    run(fda_beta=None)
    assert {k: v["launches"] for k, v in m.engine.profile_results().items()} == plain
    assert m.engine.get_option("workspace_allocations") - a1 == a1 - a0 and not hasattr(m.engine, "_fda_work")
    gc.collect(); assert torch.cuda.memory_allocated() == mem
    run(fda_beta=0.01)
    assert hasattr(m.engine, "_fda_work")
    m.close()
