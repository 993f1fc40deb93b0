"""Monte-Carlo dropout inference (fcn8s_predict_mc, include/fcn8s_hip.h): the host side of the definition.

Dropout stays on behind fc6 and fc7 at test time, S stochastic passes are drawn and their softmaxes averaged (Gal & Ghahramani 2016;
Kendall et al., "Bayesian SegNet", 2015; Kendall & Gal, "What uncertainties do we need in Bayesian deep learning for computer vision?",
2017).  Per pixel, with p_s the softmax of sample s and h(p) = -sum_c p_c log(max(p_c, FLT_MIN)):

    mean               = (sum_s p_s) * (1 / S)
    entropy            = h(mean)                                      the total predictive uncertainty
    mutual_information = max(0, entropy - (sum_s h(p_s)) * (1 / S))    its epistemic part (BALD)
    argmax of mean, lowest index on ties

`validate` is what Engine.predict_mc refuses before anything is launched, `stream_ids` names the counter streams of a sample's two masks,
`restate` evaluates the definition on the host from per-sample logits (the tests' reference)."""
import numpy as np

MAX_SAMPLES = 256                 # FCN8S_MC_MAX_SAMPLES
STREAM_BASE = 0x80000000          # training draws its masks on streams 2 step and 2 step + 1, step < 2^30: below this
MAX_SAMPLE_INDEX = 1 << 30        # sample_offset + samples may not exceed it (the stream ids stay 32-bit)
FLT_MIN = float(np.finfo(np.float32).tiny)


def validate(samples, keep_prob, sample_offset=0):
    """(samples, keep_prob, sample_offset) as (int, float, int), or ValueError / TypeError for what fcn8s_predict_mc refuses."""
    for name, v in (("samples", samples), ("sample_offset", sample_offset)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("`%s` must be an integer, got %r" % (name, v))
    samples, sample_offset = int(samples), int(sample_offset)
    if not 1 <= samples <= MAX_SAMPLES:
        raise ValueError("`samples` must lie in 1..%d, got %d" % (MAX_SAMPLES, samples))
    keep_prob = float(keep_prob)
    if not (0.0 < keep_prob <= 1.0):
        raise ValueError("`keep_prob` must lie in (0, 1], got %r" % (keep_prob,))
    if sample_offset < 0 or sample_offset + samples > MAX_SAMPLE_INDEX:
        raise ValueError("`sample_offset` must be >= 0 with sample_offset + samples <= 2^30, got %d (+ %d samples)" % (sample_offset, samples))
    return samples, keep_prob, sample_offset


def stream_ids(sample_offset, s):
    """The counter streams (fc6, fc7) of sample `s` of a call at `sample_offset`: 0x80000000 + 2 (offset + s) and that + 1."""
    k = int(sample_offset) + int(s)
    if not 0 <= k < MAX_SAMPLE_INDEX:
        raise ValueError("sample_offset + s must lie in [0, 2^30), got %d" % k)
    a = STREAM_BASE + 2 * k
    return a, a + 1


def _entropy(p, dtype):
    # h folded in class order, as the kernel's one device function: h <- h - p_c * log(max(p_c, FLT_MIN))
    h = np.zeros(p.shape[:-1], dtype)
    tiny = dtype(FLT_MIN)
    for c in range(p.shape[-1]):
        h = (h - p[..., c] * np.log(np.maximum(p[..., c], tiny))).astype(dtype)
    return h


def restate(logits_per_sample, dtype=np.float64):
    """The definition from per-sample logits [S, ..., C] (float32 values): (mean [..., C], entropy [...], mutual_information [...],
    argmax [...] int64).  dtype=np.float64 is the reference; dtype=np.float32 is the same definition in the device's operation order
    (softmax as exp(l - max) / sum with the sum folded in class order, sums folded in sample order, one multiply by the fp32 reciprocal)."""
    dtype = np.dtype(dtype).type
    x = np.asarray(logits_per_sample, np.float32).astype(dtype)
    if x.ndim < 2 or x.shape[0] < 1:
        raise ValueError("`logits_per_sample` must be [S, ..., C] with S >= 1")
    S, C = x.shape[0], x.shape[-1]
    inv = dtype(1.0) / dtype(S)
    acc = hacc = None
    for s in range(S):
        e = np.exp(x[s] - x[s].max(-1, keepdims=True)).astype(dtype)
        tot = np.zeros(e.shape[:-1], dtype)
        for c in range(C):
            tot = (tot + e[..., c]).astype(dtype)
        p = (e / tot[..., None]).astype(dtype)
        h = _entropy(p, dtype)
        acc = p if acc is None else (acc + p).astype(dtype)
        hacc = h if hacc is None else (hacc + h).astype(dtype)
    mean = (acc * inv).astype(dtype)
    ent = _entropy(mean, dtype)
    mi = np.maximum(dtype(0.0), ent - (hacc * inv).astype(dtype)).astype(dtype)
    return mean, ent, mi, np.argmax(mean, -1).astype(np.int64)
