"""FCN8s.train(focal_gamma=...) on the GPU, on batches of 2 images of 64 x 96: two updates equal the same updates driven by hand through Engine
-- set_focal -> train_step, alone; set_loss + set_boundary_loss + set_focal -> accumulate_step, train_step with `class_weights`,
`boundary_weight` and accumulation_steps = 2 -- bit for bit in every parameter; the engine's previous setting is back after a normal return and
after an exception from the generator; `ohem_thresh` together with `focal_gamma` raises before the engine is touched; and focal_gamma = 0 leaves
the step what it was."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fcn8s_tensorflow_amd import loss as LM  # noqa: E402
from tests.test_class_mix_facade_gpu import LR, batches, gen, model, params_of, same_bits  # noqa: E402

GAMMA = 2.0
CWS = np.linspace(0.5, 2.0, 20).astype(np.float32)
BOUNDARY = dict(boundary_weight=4.0, boundary_sigma=3.0)

MODES = {
    "alone": dict(A=1, kw={}),
    "weights_boundary_accumulate": dict(A=2, kw=dict(class_weights=CWS, accumulation_steps=2, **BOUNDARY)),
}


def by_hand(b, items, A, kw):
    e = b.engine
    if "class_weights" in kw:
        e.set_loss(kw["class_weights"])
        e.set_boundary_loss(*LM.resolve_boundary(kw["boundary_weight"], kw["boundary_sigma"], None, None))
    e.set_focal(GAMMA)
    terms = []
    for u in range(2):
        for k in range(A):
            img, lab = items[u * A + k]
            X, Y = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
            if k < A - 1:
                e.accumulate_step(X, Y, keep_prob=1.0, l2_rate=0.0)
            else:
                e.train_step(X, Y, LR, keep_prob=1.0, l2_rate=0.0)
        terms.append(e.loss_terms()["ce"])
    return terms


@pytest.mark.parametrize("mode", list(MODES))
def test_train_with_the_focal_loss_equals_the_updates_driven_by_hand(mode):
    cfg = MODES[mode]
    A = cfg["A"]
    items = batches(2 * A)
    run = lambda m, **kw: m.train(gen(items), epochs=1, steps_per_epoch=2, learning_rate_schedule=lambda s: LR, keep_prob=1.0, record_summaries=False,
                                  **dict(cfg["kw"], **kw))
    a = model()
    before = params_of(a)
    run(a, focal_gamma=GAMMA)
    assert a.g_step == 2 and np.isfinite(a.training_loss) and a.engine.focal_config is None and a.engine.loss_config is None
    got = params_of(a)
    assert any(np.abs(got[k] - before[k]).max() > 0 for k in got)
    a.close()

    b = model()
    terms = by_hand(b, items, A, cfg["kw"])
    want = params_of(b)
    assert all(np.isfinite(t) and t > 0 for t in terms)
    b.close()
    same_bits(got, want)

    c = model()                                                                 # and gamma has force: without it the parameters differ
    run(c)
    off = params_of(c)
    c.close()
    assert any(np.abs(got[k] - off[k]).max() > 0 for k in got)

    d = model()                                                                 # focal_gamma = 0.0 is the step as it was, bit for bit
    run(d, focal_gamma=0.0)
    same_bits(params_of(d), off)
    d.close()


def test_the_previous_setting_is_restored_after_a_return_and_after_an_exception():
    m = model()
    m.engine.set_focal(0.5)                                                     # a setting of the caller's own
    mine = dict(m.engine.focal_config)
    assert mine == dict(gamma=0.5)
    run = lambda items, **kw: m.train(gen(items), epochs=1, steps_per_epoch=len(items), learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                                      record_summaries=False, **kw)
    run(batches(1), focal_gamma=GAMMA)
    assert m.engine.focal_config == mine
    with pytest.raises(RuntimeError, match="the generator broke"):
        m.train(gen(batches(3), fail_after=1), epochs=1, steps_per_epoch=3, learning_rate_schedule=lambda s: LR, record_summaries=False,
                focal_gamma=GAMMA)
    assert m.engine.focal_config == mine
    run(batches(1))                                                             # focal_gamma = 0 leaves the caller's setting on
    assert m.engine.focal_config == mine
    with pytest.raises(ValueError):                                             # ... and that setting meets this call's OHEM up front
        run(batches(1), ohem_thresh=0.7)
    assert m.engine.focal_config == mine and m.engine.loss_config is None
    m.engine.set_focal()
    assert m.engine.focal_config is None
    # an OHEM configuration of the caller's own: focal_gamma raises up front, unless this call replaces the loss configuration
    m.engine.set_loss(ohem_thresh=0.7, ohem_min_kept=100)
    ohem = dict(m.engine.loss_config)
    step = m.engine.global_step
    with pytest.raises(ValueError):
        run(batches(1), focal_gamma=GAMMA)
    assert m.engine.global_step == step and m.engine.focal_config is None
    run(batches(1), focal_gamma=GAMMA, class_weights=CWS)
    assert m.engine.focal_config is None and m.engine.loss_config["ohem_thresh"] == ohem["ohem_thresh"]
    m.close()


def test_each_refusal():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    for kw in (dict(focal_gamma=float("nan")), dict(focal_gamma=float("inf")), dict(focal_gamma="much"), dict(focal_gamma=True), dict(focal_gamma=-1.0),
               dict(focal_gamma=8.5), dict(focal_gamma=2.0, ohem_thresh=0.7), dict(focal_gamma=0.5, ohem_thresh=0.7, class_weights=CWS)):
        with pytest.raises(ValueError):
            run(**kw)
    assert m.engine.global_step == 0 and m.engine.focal_config is None and m.engine.loss_config is None     # the engine was not touched
    for g in (float("nan"), -1.0, 9.0, "x"):
        with pytest.raises(ValueError):
            m.engine.set_focal(g)
    m.close()


def test_with_gamma_zero_nothing_new_is_launched_or_allocated():
    m = model()
    run = lambda **kw: m.train(gen(batches(1)), epochs=1, steps_per_epoch=1, learning_rate_schedule=lambda s: LR, keep_prob=1.0,
                               record_summaries=False, **kw)
    run()
    m.engine.profile(True); m.engine.profile_reset()
    run()
    plain = {k: v["launches"] for k, v in m.engine.profile_results().items()}
    allocs = m.engine.get_option("workspace_allocations")
    m.engine.profile_reset()
    run(focal_gamma=0.0)
    assert {k: v["launches"] for k, v in m.engine.profile_results().items()} == plain and "focal_xent" not in plain
    assert m.engine.get_option("workspace_allocations") == allocs
    m.engine.profile_reset()
    run(focal_gamma=GAMMA)
    prof = m.engine.profile_results()
    assert prof["focal_xent"]["launches"] == 1 and prof.get("softmax_xent", dict(launches=0))["launches"] == 0
    assert m.engine.get_option("workspace_allocations") == allocs + 2          # the per-block partials and the loss state that holds |V|
    m.close()
