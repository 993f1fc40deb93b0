#!/usr/bin/env python
"""Digests of what a build of libfcn8s_hip.so computes in the tiled loss kernels (csrc/loss_tile.h: the focal loss, the entropy term, the soft
targets) and in the training losses around them, one JSON line per case: for comparing two BUILDS of the library that are meant to compute the same
bits.  Not a test: it needs the other build.

    python tools/loss_digest.py OUT.jsonl [--full]

Op cases: fcn8s_op_focal_xent and fcn8s_op_entropy_term at P in {1, 15, 255, 256, 257, 513, 600} x (C, K) in {(2, 2), (4, 4), (19, 19), (20, 19),
(20, 20), (21, 21), (64, 64)} (the focal op has no K: its (20, 19) is its (20, 20) again), with logits and dlogits 16-byte aligned and off by one
float, with and without dlogits, the focal op without and with class weights + distance codes, the entropy op over its three pixel sets; and one
2 x 512 x 1024 x 20 case each, where every block trips more than once.  Digested: the loss or term, the bias column sums, dlogits.
Model cases: one fresh engine (fp32, the model tests' small widths, option deterministic = 1) through two training steps (SGD, keep_prob 0.5, l2 1e-3)
at 2 x 64 x 96 and 1 x 32 x 32 with tconv_gemm 0 and 1, for the default loss, class weights, OHEM, the Lovasz term, the focal loss, the entropy term,
soft targets with K = 20, with K = 19 in rows of 20, and on models of 24 and of 12 classes (the generic 16-byte path of the soft-target kernel).
Digested: both losses, the loss terms, every gradient of step 2 and the flat parameters after it.

The file keeps one SHA-256 per case (--full: every digest as well, in OUT.jsonl.full, to find WHICH output moved).  Run it with one build in place, then with the other (copy
the .so into place as tools/ab_libs.sh does), one process each, and diff the two files.  Before it writes anything the tool checks that it has force:
with a second seed every value digest of every op case and of every loss configuration changes."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fcn8s_tensorflow_amd import _lib as L  # noqa: E402
from fcn8s_tensorflow_amd.engine import Engine  # noqa: E402
from oracle import fcn8s_oracle as orc  # noqa: E402  (the initializer only)

PS = (1, 15, 255, 256, 257, 513, 600)
CKS = ((2, 2), (4, 4), (19, 19), (20, 19), (20, 20), (21, 21), (64, 64))
BIG = (2, 512 * 1024, 20)                              # N, HW, C
SETS = ('unlabeled', 'valid', 'all')                   # FCN8S_ENT_* 0, 1, 2
SMALL = (8, 16, 32, 64, 64, 128, 128)                  # the model tests' small widths
SHAPES = ((2, 64, 96), (1, 32, 32))
CONFIGS = ('default', 'class_weights', 'ohem', 'lovasz', 'focal', 'entropy', 'kd20', 'kd19of20', 'kd24', 'kd12')


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def shifted(a, off):
    """A device copy of the float array whose first element lies `off` floats behind a 16-byte boundary."""
    import torch
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def op_inputs(npix, Cn, seed, need):
    """Logits, a dlogits to start from, labels (30 % ignored; pixel 0 ignored and pixel 1 valid, or with one pixel what `need` asks for, so that no
    pixel set is empty), codes, class weights and the table."""
    rng = np.random.default_rng([seed, npix, Cn])
    z = (3.0 * rng.standard_normal((npix, Cn))).astype(np.float32)
    d0 = rng.standard_normal((npix, Cn)).astype(np.float32)
    lab = rng.integers(0, Cn, npix, dtype=np.uint8)
    lab[rng.random(npix) < 0.3] = 255
    if npix > 1:
        lab[0], lab[1] = 255, lab[1] if lab[1] < Cn else 0
    else:
        lab[0] = 255 if need == 'unlabeled' else (lab[0] if lab[0] < Cn else 0)
    codes = rng.integers(0, 256, npix, dtype=np.uint8)
    cw = rng.uniform(0.5, 2.0, Cn).astype(np.float32)
    table = rng.uniform(0.5, 2.5, 256).astype(np.float32)
    return z, d0, lab, codes, cw, table


def focal_case(n, hw, Cn, off, with_d, weighted, seed, work):
    import torch
    npix = n * hw
    z, d0, lab, codes, cw, table = op_inputs(npix, Cn, seed, 'valid')
    zt, dt = shifted(z, off), shifted(d0, off) if with_d else None
    lt = torch.from_numpy(lab).cuda()
    ct, wt, tt = (torch.from_numpy(x).cuda() for x in (codes, cw, table)) if weighted else (None, None, None)
    loss = torch.zeros(1, device="cuda"); bias = torch.zeros(Cn, device="cuda")
    L.check(L.lib.fcn8s_op_focal_xent(None, ptr(zt), ptr(lt), ptr(wt), ptr(ct), ptr(tt), 2.0, ptr(dt), ptr(loss), ptr(bias), npix, Cn, ptr(work),
                                      work.numel()))
    out = dict(loss=sha(loss.cpu().numpy()), bias=sha(bias.cpu().numpy()))
    if with_d:
        out["dlogits"] = sha(dt.cpu().numpy())
    return out


def entropy_case(n, hw, Cn, K, off, with_d, pset, seed, work):
    import torch
    npix = n * hw
    z, d0, lab, _, _, _ = op_inputs(npix, Cn, seed, SETS[pset])
    zt, dt = shifted(z, off), shifted(d0, off) if with_d else None
    lt = torch.from_numpy(lab).cuda()
    term = torch.zeros(1, device="cuda"); bias = torch.zeros(Cn, device="cuda")
    L.check(L.lib.fcn8s_op_entropy_term(None, ptr(zt), ptr(dt), ptr(lt), n, hw, Cn, K, pset, 0, 0.5, ptr(work), work.numel(), ptr(term), ptr(bias)))
    out = dict(term=sha(term.cpu().numpy()), bias=sha(bias.cpu().numpy()))
    if with_d:
        out["dlogits"] = sha(dt.cpu().numpy())
    return out


def op_cases(seed, big):
    import torch
    fwork = torch.empty(int(L.lib.fcn8s_op_focal_xent_work_bytes()), dtype=torch.uint8, device="cuda")
    ework = torch.empty(int(L.lib.fcn8s_op_entropy_term_work_bytes()), dtype=torch.uint8, device="cuda")
    out = {}
    for P in PS:
        for Cn, K in CKS:
            for off in (0, 1):
                for with_d in (1, 0):
                    tail = "P%d/C%d/K%d/off%d/d%d" % (P, Cn, K, off, with_d)
                    for weighted in (0, 1):
                        out["focal/%s/w%d" % (tail, weighted)] = focal_case(1, P, Cn, off, with_d, weighted, seed, fwork)
                    if K >= 2:
                        for pset in range(3):
                            out["entropy/%s/%s" % (tail, SETS[pset])] = entropy_case(1, P, Cn, K, off, with_d, pset, seed, ework)
    if big:
        n, hw, Cn = BIG
        out["focal/2x512x1024x20"] = focal_case(n, hw, Cn, 0, 1, 1, seed, fwork)
        out["entropy/2x512x1024x20"] = entropy_case(n, hw, Cn, Cn, 0, 1, 2, seed, ework)
    return out


def soft_rows(shape, K, seed):
    rng = np.random.default_rng(seed)
    z = 4.0 * rng.standard_normal(shape + (K,))
    p = np.exp(z - z.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def model_case(config, shape, tconv_gemm, seed):
    import torch
    nc, logical = {'kd24': (24, 24), 'kd12': (12, 12), 'kd19of20': (20, 19)}.get(config, (20, 20))
    rng = np.random.default_rng(1000 + seed)
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    lab = rng.integers(0, logical, shape, dtype=np.uint8)
    lab[rng.random(shape) < 0.1] = 255
    e = Engine(nc, widths=SMALL, device_id=0, seed=0, logical_classes=logical, options=dict(tconv_gemm=tconv_gemm, deterministic=1))
    e.set_params(orc.init_params(logical, SMALL, seed=seed, decoder_std_scale=3.0, bias_std=0.05))
    if config == 'class_weights':
        e.set_loss(class_weights=np.random.default_rng(7).uniform(0.5, 2.0, 20).astype(np.float32))
    elif config == 'ohem':
        e.set_loss(ohem_thresh=0.7, ohem_min_kept=100)
    elif config == 'lovasz':
        e.set_lovasz(0.5)
    elif config == 'focal':
        e.set_focal(2.0)
    elif config == 'entropy':
        e.set_entropy_term(0.5, 'all')
    elif config.startswith('kd'):
        e.set_soft_targets(0.7, 2.0, 'valid')
    out = {"loss": [], "terms": []}
    for step in range(2):
        if config.startswith('kd'):
            rows = torch.from_numpy(soft_rows(shape, logical, 100 * seed + step)).cuda()
            if config == 'kd19of20':                   # rows of 19 in strides of 20: a class slice of a wider tensor
                wide = torch.full(shape + (20,), float("nan"), device="cuda")
                wide[..., :19] = rows
                rows = wide[..., :19]
            e.bind_soft_targets(rows)
        loss, _ = e.train_step(img, lab, 1e-3, keep_prob=0.5, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        terms = e.loss_terms()
        if config.startswith('kd'):
            terms["kd"] = e.soft_target_term()
        if config == 'entropy':
            terms["entropy"] = e.entropy_term()
        out["loss"].append(sha(np.float32(loss)))
        out["terms"].append({k: sha(np.float32(v)) for k, v in sorted(terms.items())})
    grads = e.get_grads()
    out["grads"] = {k: sha(g) for k, g in grads.items()}
    out["params"] = sha(e.flat_params.detach().cpu().numpy())
    e.close()
    return out, {"/grads/" + k for k, g in grads.items() if not g.any()}       # (a gradient of zeros is the same under every seed)


def leaves(x, path=""):
    if isinstance(x, dict):
        for k in sorted(x):
            yield from leaves(x[k], path + "/" + str(k))
    elif isinstance(x, list):
        for i, v in enumerate(x):
            yield from leaves(v, path + "/" + str(i))
    else:
        yield path, x


def main(path, full=False):
    lines = op_cases(1, True)
    print("%d op cases" % len(lines), flush=True)
    for config in CONFIGS:
        for shape in SHAPES:
            for tg in (0, 1):
                lines["model/%s/%dx%dx%d/tconv_gemm=%d" % ((config,) + shape + (tg,))] = model_case(config, shape, tg, 1)[0]
        print(config, flush=True)
    # the tool has force: another seed, another digest, for every value (the terms that are switched off are 0 under every seed)
    other = op_cases(2, False)
    for name, v in other.items():
        for k in v:
            assert v[k] != lines[name][k], ("another seed, the same digest", name, k)
    for config in CONFIGS:
        name = "model/%s/%dx%dx%d/tconv_gemm=1" % ((config,) + SHAPES[1])
        second, zeros = model_case(config, SHAPES[1], 1, 2)
        a, b = dict(leaves(lines[name])), dict(leaves(second))
        assert a.keys() == b.keys()
        for k in a:
            off = (k.endswith("/lovasz") and config != 'lovasz') or k in zeros
            assert off or a[k] != b[k], ("another seed, the same digest", name, k)
    with open(path, "w") as f:
        for name in sorted(lines):
            f.write(json.dumps({"case": name, "values": hashlib.sha256(json.dumps(lines[name], sort_keys=True).encode()).hexdigest()}) + "\n")
    if full:
        with open(path + ".full", "w") as f:
            for name in sorted(lines):
                f.write(json.dumps({"case": name, "values": lines[name]}, sort_keys=True) + "\n")
    print("%d cases -> %s" % (len(lines), path))


if __name__ == "__main__":
    main(sys.argv[1], "--full" in sys.argv[2:])
