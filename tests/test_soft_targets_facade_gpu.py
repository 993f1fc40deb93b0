"""FCN8s.train(teacher=...) on the GPU: three updates of a narrow student under a wide teacher equal the same updates driven by hand through Engine
(predict, bind_soft_targets, train_step), bit for bit -- with the plain teacher, with `teacher_predict` (flip averaging), with a callable teacher and
with accumulation_steps=2; the teacher's frozen state and the student's soft-target setting are restored after a normal return and after an exception
raised inside the generator; `distill_loss` joins the recorded scalars."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NARROW = (8, 16, 32, 64, 64, 128, 128)
WIDE = (16, 32, 64, 128, 128, 256, 256)
SHAPE = (2, 32, 64)
LR, WEIGHT, TEMP = 1e-3, 0.7, 2.0


def batches(count, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        img = rng.integers(0, 256, SHAPE + (3,), dtype=np.uint8)
        lab = rng.integers(0, 20, SHAPE, dtype=np.uint8)
        lab[rng.random(SHAPE) < 0.1] = 255
        out.append((img, lab))
    return out


def gen(items, fail_after=None):
    for k, item in enumerate(items):
        if fail_after is not None and k == fail_after:
            raise RuntimeError("the generator broke")
        yield item


def student():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    m = FCN8s(vgg16_dir='synthetic:3', num_classes=20, widths=NARROW)
    m.engine.set_option("deterministic", 1)
    return m


@functools.lru_cache(maxsize=None)
def wide_teacher():
    from fcn8s_tensorflow_amd.fcn8s import FCN8s
    T = FCN8s(vgg16_dir='synthetic:5', num_classes=20, widths=WIDE)
    # a freshly initialised decoder predicts almost uniformly, as the student's does: KL ~ 0 and the term would have no force.  An opinionated last bias
    # gives the teacher a distribution the student does not have
    T.engine.set_params({"fc7_pool4_pool3_conv2d_trans/bias": np.linspace(-2.0, 2.0, 20).astype(np.float32)})
    return T


def params_of(m):
    return {k: v.copy() for k, v in m.engine.get_params().items()}


MODES = {
    "model": (dict(), lambda T, x: T.engine.predict(x, argmax=False), 1),
    "flip": (dict(teacher_predict=dict(scales=(1.0,), flip=True)), lambda T, x: T.engine.predict_tta(x, scales=(1.0,), flip=True, argmax=False), 1),
    "callable": (dict(), lambda T, x: T.engine.predict(x, argmax=False), 1),
    "accumulate": (dict(accumulation_steps=2), lambda T, x: T.engine.predict(x, argmax=False), 2),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_train_with_a_teacher_equals_the_updates_driven_by_hand(mode):
    kw, by_hand_teacher, A = MODES[mode]
    T = wide_teacher()
    items = batches(3 * A)
    a = student()
    before = params_of(a)
    teacher = (lambda x: T.engine.predict(x, argmax=False)) if mode == "callable" else T
    a.train(gen(items), epochs=1, steps_per_epoch=3, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
            teacher=teacher, distill_weight=WEIGHT, distill_temperature=TEMP, **kw)
    assert a.g_step == 3 and np.isfinite(a.training_loss) and a.engine.soft_target_config is None
    got = params_of(a)
    assert any(np.abs(got[k] - before[k]).max() > 0 for k in got)
    a.close()

    b = student()
    e = b.engine
    e.set_soft_targets(WEIGHT, TEMP, 'valid')
    for u in range(3):
        for k in range(A):
            img, lab = items[u * A + k]
            dev = torch.from_numpy(img).cuda()
            e.bind_soft_targets(by_hand_teacher(T, dev))
            if k < A - 1:
                e.accumulate_step(dev, lab, keep_prob=1.0, l2_rate=0.0)
            else:
                e.train_step(dev, lab, LR, keep_prob=1.0, l2_rate=0.0)
    want = params_of(b)
    b.close()
    for k in want:
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)


def test_a_teacher_changes_the_training_and_weight_zero_does_not():
    T = wide_teacher()
    items = batches(2)
    res = []
    for kw in (dict(), dict(teacher=T, distill_weight=0.0), dict(teacher=T, distill_weight=1.0, distill_pixels='all')):
        m = student()
        m.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False, **kw)
        res.append(params_of(m))
        m.close()
    for k in res[0]:
        np.testing.assert_array_equal(res[0][k].view(np.uint32), res[1][k].view(np.uint32), err_msg=k)
    assert any(np.abs(res[0][k] - res[2][k]).max() > 0 for k in res[0])


@pytest.mark.parametrize("teacher_frozen", [False, True])
def test_settings_are_restored_after_a_return_and_after_an_exception(teacher_frozen, tmp_path):
    T = wide_teacher()
    T.engine.freeze(teacher_frozen)
    m = student()
    m.engine.set_soft_targets(0.3, 4.0, 'all')                              # a setting of the caller's own
    mine = dict(m.engine.soft_target_config)
    m.train(gen(batches(2)), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, summaries_dir=str(tmp_path),
            summaries_frequency=1, teacher=T, distill_weight=WEIGHT, distill_temperature=TEMP, teacher_predict=dict(temperature=1.5))
    assert m.engine.soft_target_config == mine and bool(T.engine.get_option("frozen")) == teacher_frozen
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path), 'training', 'scalars.jsonl'))]
    assert len(rows) == 2 and all(np.isfinite(r["distill_loss"]) and r["distill_loss"] > 0 for r in rows)
    with pytest.raises(RuntimeError, match="the generator broke"):
        m.train(gen(batches(3), fail_after=1), epochs=1, steps_per_epoch=3, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                record_summaries=False, teacher=T, distill_weight=WEIGHT, accumulation_steps=1)
    assert m.engine.soft_target_config == mine and bool(T.engine.get_option("frozen")) == teacher_frozen
    with pytest.raises(Exception):                                          # the caller's own setting is on and nothing is bound
        m.engine.train_step(*batches(1)[0], LR)
    m.engine.set_soft_targets()
    T.engine.freeze(False)
    m.close()


def test_teacher_arguments_are_checked():
    T = wide_teacher()
    m = student()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, record_summaries=False, **kw)
    for kw in (dict(teacher=m), dict(teacher=3), dict(teacher_predict=dict(flip=True)), dict(teacher=T, distill_weight=-1.0),
               dict(teacher=T, distill_temperature=0.0), dict(teacher=T, distill_pixels='some'), dict(teacher=T, teacher_predict=dict(argmax=True)),
               dict(teacher=T, teacher_predict=dict(samples=2, flip=True)), dict(teacher=lambda x: x, teacher_predict=dict(flip=True))):
        with pytest.raises(ValueError):
            run(**kw)
    with pytest.raises(ValueError):                                          # a callable that returns something else than a device softmax
        run(teacher=lambda x: x)
    assert m.engine.soft_target_config is None and m.engine.global_step == 0
    run(teacher=T, teacher_predict=dict(samples=2, keep_prob=0.5))           # the Monte-Carlo mean as the target
    assert m.engine.global_step == 1
    m.close()
