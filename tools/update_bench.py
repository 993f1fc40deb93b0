#!/usr/bin/env python3
"""The update's streaming kernels (csrc/optim.hip) at full width -- the 538 MB gradient buffer -- and what accumulation and the clip add
to a training step at 16 x 1024x512, in one process:

  * kernels (device events around --reps back-to-back launches, --rounds rounds, every candidate timed in every round next to a
    device-to-device copy that moves the same number of bytes; the row holds the medians over the rounds and their ratio):
      fold_first   acc = g        over all buckets   8 B / element   against a copy of n floats
      fold         acc += g       over all buckets  12 B / element   against a copy of 1.5 n floats
      flush        g += acc       over all buckets  12 B / element   against the same copy
      grad_norm    partial sums + finalize           4 B / element   against a copy of n / 2 floats
    TARGET: each within 1.25 x its copy.
  * update: fcn8s_apply_update (TF-Adam) with the clip off and with max_norm = inf, alternating, and -- from a profiled run of its own --
    the `adam` and `grad_norm` profile groups of both.
  * step: ms per update at 16 x 1024x512 (device inputs), fp32 and bf16_train, alternating A = 1 clip off / A = 1 clip = inf /
    A = 2 clip off (two micro-batches of 16 images per update).

Prints one JSON line per row and writes them to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, NC = 16, 512, 1024, 20
TARGET = 1.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--precisions", default="fp32,bf16_train")
    ap.add_argument("--widths", default=None, help="seven comma-separated channel widths (default: the full network)")
    ap.add_argument("--batch", type=int, default=N)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("update_bench.py needs an MI355X: nothing is measured without one")
    widths = tuple(int(x) for x in a.widths.split(",")) if a.widths else None
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn, reps):
        """ms per call of fn over `reps` back-to-back calls, by device events"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    def alternate(cands, reps, rounds, warmup):
        """{name: fn} -> {name: [ms per round]}: every candidate warmed up, then timed once per round, in turn"""
        for fn in cands.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        out = {k: [] for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                out[k].append(timed(fn, reps))
        return out

    med = lambda v: float(np.median(v))

    e = Engine(NC, widths=widths, device_id=0, seed=0)
    e.init_params(0)
    n = e.flat_grads.numel()
    g = torch.Generator(device="cuda").manual_seed(0)
    e.flat_grads.copy_(torch.randn(n, device="cuda", generator=g) * 1e-3)
    acc = torch.zeros(n, device="cuda")
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def accumulate(dst, src, mode):
        def run():
            s = stream()
            for off, cnt in e.buckets:
                L.check(L.lib.fcn8s_op_grad_accumulate(s, C.c_void_p(dst.data_ptr() + 4 * off), C.c_void_p(src.data_ptr() + 4 * off), cnt, mode))
        return run

    def copier(floats):
        src = torch.empty(floats, device="cuda").normal_(generator=g)
        dst = torch.empty(floats, device="cuda")
        return lambda: dst.copy_(src)

    e.set_grad_clip(float("inf"))
    norm_only = lambda: e.apply_update(1e-6, optimizer=L.OPT_NONE)           # clip on, no optimizer: the norm pass and its finalize kernel
    kernels = (("fold_first", accumulate(acc, e.flat_grads, 0), 8, n), ("fold", accumulate(acc, e.flat_grads, 1), 12, n + n // 2),
               ("flush", accumulate(e.flat_grads, acc, 1), 12, n + n // 2), ("grad_norm", norm_only, 4, n // 2))
    for name, fn, bpe, copy_floats in kernels:
        if name == "flush":
            acc.zero_()                                                       # (g += 0: the gradient keeps its values over the repetitions)
        r = alternate({"kernel": fn, "copy": copier(copy_floats)}, a.reps, a.rounds, a.warmup)
        k, c = med(r["kernel"]), med(r["copy"])
        emit(dict(kind="kernel", name=name, elements=n, bytes=bpe * n, kernel_ms=round(k, 4), copy_ms=round(c, 4), copy_bytes=8 * copy_floats,
                  ratio=round(k / c, 3), target=TARGET, within_target=bool(k <= TARGET * c), kernel_tbps=round(bpe * n / k / 1e9, 3),
                  copy_tbps=round(8 * copy_floats / c / 1e9, 3), kernel_ms_rounds=[round(x, 4) for x in r["kernel"]],
                  copy_ms_rounds=[round(x, 4) for x in r["copy"]], reps=a.reps, launches_per_call=len(e.buckets) if name != "grad_norm" else 2))
    del acc
    torch.cuda.empty_cache()

    # the update with and without the clip
    def update(clip):
        def run():
            e.set_grad_clip(clip)
            e.apply_update(1e-6)
        return run
    r = alternate({"clip_off": update(None), "clip_inf": update(float("inf"))}, a.reps, a.rounds, a.warmup)
    prof = {}
    for name, clip in (("clip_off", None), ("clip_inf", float("inf"))):
        e.set_grad_clip(clip)
        e.profile(True); e.profile_reset()
        for _ in range(5):
            e.apply_update(1e-6)
        torch.cuda.synchronize()
        res = e.profile_results()
        prof[name] = {k: round(res[k]["ms"] / 5, 4) for k in ("adam", "grad_norm") if k in res and res[k]["launches"]}
        e.profile(False)
    off, on = med(r["clip_off"]), med(r["clip_inf"])
    emit(dict(kind="update", optimizer="tf_adam", elements=n, clip_off_ms=round(off, 4), clip_inf_ms=round(on, 4), added_ms=round(on - off, 4),
              ratio=round(on / off, 3), profile_groups_ms=prof, clip_off_ms_rounds=[round(x, 4) for x in r["clip_off"]],
              clip_inf_ms_rounds=[round(x, 4) for x in r["clip_inf"]], reps=a.reps))
    e.set_grad_clip(None)
    e.close()
    del e
    torch.cuda.empty_cache()

    # the training step
    Nb, Hh, Ww = a.batch, a.height, a.width
    for precision in a.precisions.split(","):
        e = Engine(NC, widths=widths, device_id=0, seed=0, precision=precision)
        e.init_params(0)
        img = torch.randint(0, 256, (Nb, Hh, Ww, 3), dtype=torch.uint8, device="cuda", generator=g)
        lab = torch.randint(0, NC, (Nb, Hh, Ww), dtype=torch.uint8, device="cuda", generator=g)

        def a1(clip):
            def run():
                if e.grad_clip != clip:
                    e.set_grad_clip(clip)
                e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False)
            return run

        def a2():
            if e.grad_clip is not None:
                e.set_grad_clip(None)
            e.accumulate_step(img, lab, keep_prob=0.5, fetch_loss=False)
            e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False)
        r = alternate({"a1_clip_off": a1(None), "a1_clip_inf": a1(float("inf")), "a2_clip_off": a2}, a.steps, a.rounds, a.warmup)
        allocs0 = e.get_option("workspace_allocations")
        base = med(r["a1_clip_off"])
        emit(dict(kind="step", precision=precision, batch="%dx%dx%d" % (Nb, Ww, Hh), a1_clip_off_ms=round(base, 3),
                  a1_clip_inf_ms=round(med(r["a1_clip_inf"]), 3), a2_update_ms=round(med(r["a2_clip_off"]), 3),
                  a2_per_micro_batch_ms=round(med(r["a2_clip_off"]) / 2, 3), clip_added_ms=round(med(r["a1_clip_inf"]) - base, 3),
                  accumulation_added_ms_per_update=round(med(r["a2_clip_off"]) - 2 * base, 3),
                  rounds={k: [round(x, 3) for x in v] for k, v in r.items()}, steps_per_round=a.steps, workspace_allocations=allocs0))
        e.close()
        del e, img, lab
        torch.cuda.empty_cache()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
