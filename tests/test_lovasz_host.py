"""The Lovász-softmax restatement (loss.py) against a literal float64 torch transcription of the published lovasz_softmax / lovasz_grad
(Berman, Rannen Triki, Blaschko, CVPR 2018) with autograd for the gradients; the closed-form Jaccard gradient against the cumulative-sum
form at 8 M labels; and the argument validation that mirrors fcn8s_set_lovasz."""
import numpy as np
import pytest
import torch

from fcn8s_tensorflow_amd import loss as LM


# ---- the published code, transcribed (float64, stable sort: the tie rule of the definition) ------------------------------------------
def _lovasz_grad(gt_sorted):
    p = len(gt_sorted)
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.double().cumsum(0)
    union = gts + (1 - gt_sorted).double().cumsum(0)
    jaccard = 1. - intersection / union
    if p > 1:
        jaccard[1:p] = jaccard[1:p] - jaccard[0:-1]
    return jaccard


def _lovasz_softmax_flat(probas, labels, classes='present'):
    if probas.numel() == 0:
        return probas.sum() * 0.          # (the published code returns probas * 0.; a scalar keeps the per-image mean defined)
    C = probas.size(1)
    losses = []
    class_to_sum = list(range(C)) if classes in ['all', 'present'] else classes
    for c in class_to_sum:
        fg = (labels == c).double()
        if classes == 'present' and fg.sum() == 0:
            continue
        class_pred = probas[:, c]
        errors = (fg - class_pred).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        fg_sorted = fg[perm]
        losses.append(torch.dot(errors_sorted, _lovasz_grad(fg_sorted)))
    if not losses:
        return probas.sum() * 0.
    return sum(losses) / len(losses)


def _flatten(probas, labels, C):
    valid = labels < C
    return probas[valid], labels[valid]


def reference(x, labels, N, per_image, classes, is_logits):
    """-> (loss, d loss / d x) by autograd; x (P, C) float64 logits or probabilities."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    C = xt.shape[1]
    probas = torch.softmax(xt, 1) if is_logits else xt
    lab = torch.tensor(np.asarray(labels).reshape(-1).astype(np.int64))
    if per_image:
        L = xt.shape[0] // N
        loss = sum(_lovasz_softmax_flat(*_flatten(probas[i * L:(i + 1) * L], lab[i * L:(i + 1) * L], C), classes) for i in range(N)) / N
    else:
        loss = _lovasz_softmax_flat(*_flatten(probas, lab, C), classes)
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


def _case(kind, seed, N=3, L=400, C=6):
    rng = np.random.default_rng(seed)
    P = N * L
    z = rng.standard_normal((P, C)) * 2
    lab = rng.integers(0, C, P)
    lab[rng.random(P) < 0.1] = 255
    if kind == "ties":
        z = np.round(z)                                    # few distinct logit rows: massive ties in the errors
        lab = rng.integers(0, 2, P) * 2
    elif kind == "absent":
        lab[lab == 2] = 255; lab[lab == 4] = 0
    elif kind == "ignored_image":
        lab[L:2 * L] = 255
    elif kind == "single":
        lab[:] = 255; lab[7] = 1
    return z, lab


def _probs(z):
    p = np.exp(z - z.max(1, keepdims=True))
    return p / p.sum(1, keepdims=True)


@pytest.mark.parametrize("kind", ["random", "ties", "absent", "ignored_image", "single"])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", ["present", "all", [0, 2, 5]])
def test_restatement_matches_published_code(kind, per_image, classes):
    z, lab = _case(kind, 11)
    N = 3
    for is_logits in (True, False):
        # (probabilities: multiples of 2^-20, so that fp32 holds them and 1 - p exactly, as the restatement takes the errors in fp32)
        x = z if is_logits else np.round(_probs(z) * 2.0 ** 20) / 2.0 ** 20
        ref_loss, ref_grad = reference(x, lab, N, per_image, classes, is_logits)
        r = LM.lovasz_restate(x, lab, N, per_image=per_image, classes=classes, x_is='logits' if is_logits else 'probs')
        assert abs(r["loss"] - ref_loss) <= 1e-12 * max(1.0, abs(ref_loss)), (r["loss"], ref_loss)
        g = r["grad_logits"] if is_logits else r["grad_prob"]
        assert np.abs(g - ref_grad).max() <= 1e-9 * max(np.abs(ref_grad).max(), 1e-300)


def test_probabilities_exactly_zero_and_one():
    rng = np.random.default_rng(3)
    P, C = 300, 4
    lab = rng.integers(0, C, P)
    p = np.zeros((P, C))
    hot = np.where(rng.random(P) < 0.5, lab, rng.integers(0, C, P))     # half the pixels certain and right, the rest certain and wrong
    p[np.arange(P), hot] = 1.0
    for per_image in (False, True):
        ref_loss, ref_grad = reference(p, lab, 3, per_image, "present", False)
        r = LM.lovasz_restate(p, lab, 3, per_image=per_image, x_is='probs')
        assert abs(r["loss"] - ref_loss) <= 1e-12 * max(1.0, ref_loss)
        assert np.abs(r["grad_prob"] - ref_grad).max() <= 1e-9 * np.abs(ref_grad).max()


def test_class_losses_and_participation():
    z, lab = _case("absent", 5)
    r = LM.lovasz_restate(z, lab, 3, per_image=True, classes="present")
    for s in range(3):
        seg = lab[s * 400:(s + 1) * 400]
        present = np.array([(seg == c).any() for c in range(6)])
        np.testing.assert_array_equal(r["participating"][s], present)
        assert (r["class_loss"][s][~present] == 0).all()
    ra = LM.lovasz_restate(z, lab, 3, per_image=False, classes="all")
    assert ra["participating"].all()
    assert abs(ra["loss"] - ra["class_loss"].mean()) <= 1e-15


def test_closed_form_matches_cumsum_form_at_8m_labels():
    rng = np.random.default_rng(0)
    fg = rng.random(8 * 1024 * 1024) < 0.05
    e = rng.random(fg.size)
    order = np.argsort(-e, kind="stable")
    a, b = LM.lovasz_grad(fg[order]), LM.lovasz_grad_cumsum(fg[order])
    assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
    la, lb = float(np.dot(e[order], a)), float(np.dot(e[order], b))
    assert abs(la - lb) <= 1e-9 * abs(la)
    # the fp32 cumulative-sum form (the published code on fp32 tensors) is the one that breaks down; the closed form does not use it
    f32 = torch.tensor(fg[order]).float()
    gts = f32.sum()
    j = 1. - (gts - f32.cumsum(0)) / (gts + (1 - f32).cumsum(0))
    j[1:] = j[1:] - j[:-1].clone()
    bg = ~fg[order]
    rel = np.abs(j.numpy()[bg] - a[bg]) / a[bg].clip(1e-300)
    assert (rel > 0.1).mean() > 0.1


def test_single_valid_pixel_and_empty_segment():
    z = np.zeros((8, 4)); lab = np.full(8, 255); lab[3] = 2
    r = LM.lovasz_restate(z, lab, 2, per_image=True, classes="present")
    # image 0 holds one foreground pixel of class 2 (e = 0.75, g = 1); image 1 has no valid pixel and counts as 0
    assert abs(r["loss"] - 0.75 / 2) <= 1e-15


@pytest.mark.parametrize("kw", [dict(lovasz_weight=-1.0), dict(lovasz_weight=float("nan")), dict(lovasz_weight=float("inf")),
                                dict(lovasz_weight=1.0, ce_weight=-0.5), dict(lovasz_weight=0.0, ce_weight=0.0),
                                dict(lovasz_weight=1.0, per_image=2), dict(lovasz_weight=1.0, classes="some"),
                                dict(lovasz_weight=1.0, classes=[]), dict(lovasz_weight=1.0, classes=[0, 19]),
                                dict(lovasz_weight=1.0, classes=[-1]), dict(lovasz_weight="x")])
def test_validate_rejects_what_the_abi_rejects(kw):
    with pytest.raises(ValueError):
        LM.validate_lovasz(num_classes=19, **kw)


def test_validate_builds_the_mask():
    ce, lov, pi, ca, m = LM.validate_lovasz(0.5, 1.0, True, [1, 3], num_classes=5)
    assert (ce, lov, pi, ca) == (1.0, 0.5, 1, 1) and m.tolist() == [0, 1, 0, 1, 0]
    assert LM.validate_lovasz(1.0, num_classes=3)[3:][0] == 0
    assert LM.validate_lovasz(1.0, classes="all", num_classes=3)[3] == 1
