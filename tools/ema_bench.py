#!/usr/bin/env python3
"""The parameter average (csrc/optim.hip, "the average" in include/fcn8s_hip.h) at full width -- 538 MB buffers -- in one process, by
device events: one untimed warm-up pass over every variant, then --rounds (at least 20) alternating repetitions, every variant timed
once per round in turn.

  * update, per optimizer (TF-Adam, SGD-momentum), on the op-level entry points over the model's own buffers:
      off        fcn8s_op_tf_adam / fcn8s_op_sgd_momentum          28 / 20 B per element   (the kernels that run without an average)
      fused      fcn8s_op_tf_adam_ema / fcn8s_op_sgd_momentum_ema  36 / 28 B per element
      unfused    off + fcn8s_op_ema_update                         40 / 32 B per element
    From bytes alone (estimates, not measurements): fused / off = 1.29 (Adam), 1.4 (SGD); unfused / off = 1.43, 1.6.
    WHAT MUST HOLD: fused < unfused in the same run (row field `fused_faster`).
  * --baseline-lib PATH: a second copy of the library (a build of another commit, outside the tree's own) is loaded with the prototypes of
    _lib.py.  Its off and fused forms are timed in the same rounds ("baseline_off", "baseline_fused"), and theta, m, v (and s) after one
    step of either library from identical inputs are compared with == at full width (rows of kind "bits_vs_baseline").
    WHAT MUST HOLD: per optimizer, off and fused, this tree's median <= the baseline's median + the baseline's own min-max spread over the
    rounds (rows of kind "vs_baseline", field `no_slower`), and every `equal` is true; the exit status says so.
  * swap       fcn8s_op_swap, 16 B per element.
  * step       Engine.train_step at 16 x 1024x512 (device inputs, fp32) with the average off and on, alternating.

Prints one JSON line per row (medians, the min-max spread of the rounds, the ratios) and writes them to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, NC = 16, 512, 1024, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5, help="back-to-back launches per timed repetition (kernels)")
    ap.add_argument("--steps", type=int, default=2, help="train steps per timed repetition")
    ap.add_argument("--step-rounds", type=int, default=20)
    ap.add_argument("--widths", default=None, help="seven comma-separated channel widths (default: the full network)")
    ap.add_argument("--batch", type=int, default=N)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--baseline-lib", default=None, help="libfcn8s_hip.so of another build to time and compare the updates against")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 20 or a.step_rounds < 20:
        raise SystemExit("ema_bench.py: at least 20 alternating repetitions")
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench.py needs an MI355X: nothing is measured without one")
    widths = tuple(int(x) for x in a.widths.split(",")) if a.widths else None
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    def alternate(cands, reps, rounds):
        for fn in cands.values():                 # one untimed warm-up pass over every variant
            fn()
        torch.cuda.synchronize()
        out = {k: [] for k in cands}
        for _ in range(rounds):
            for k, fn in cands.items():
                out[k].append(timed(fn, reps))
        return out

    def stats(v):
        return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(np.min(v)), 4), max_ms=round(float(np.max(v)), 4))

    def ratio_spread(num, den):
        r = np.asarray(num) / np.asarray(den)     # per round: the two were timed next to each other
        return dict(median=round(float(np.median(r)), 4), min=round(float(np.min(r)), 4), max=round(float(np.max(r)), 4))

    e = Engine(NC, widths=widths, device_id=0, seed=0)
    e.init_params(0)
    n = e.flat_params.numel()
    g = torch.Generator(device="cuda").manual_seed(0)
    e.flat_grads.copy_(torch.randn(n, device="cuda", generator=g) * 1e-3)
    m, v, s = (torch.zeros(n, device="cuda") for _ in range(3))
    s.copy_(e.flat_params)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    th, gr = e.flat_params, e.flat_grads
    w = 1e-3
    lr = 1e-9                                     # (the parameters stay where they are over the repetitions)

    adam_off = lambda: L.check(L.lib.fcn8s_op_tf_adam(stream(), p(th), p(gr), p(m), p(v), n, 1000, lr, 0.9, 0.999, 1e-8, 1.0))
    adam_fused = lambda: L.check(L.lib.fcn8s_op_tf_adam_ema(stream(), p(th), p(gr), p(m), p(v), p(s), n, 1000, lr, 0.9, 0.999, 1e-8, 1.0, None, w))
    sgd_off = lambda: L.check(L.lib.fcn8s_op_sgd_momentum(stream(), p(th), p(gr), p(m), n, lr, 0.9, 1.0))
    sgd_fused = lambda: L.check(L.lib.fcn8s_op_sgd_momentum_ema(stream(), p(th), p(gr), p(m), p(s), n, lr, 0.9, 1.0, None, w))
    ema = lambda: L.check(L.lib.fcn8s_op_ema_update(stream(), p(s), p(th), n, w, None))
    B = None
    if a.baseline_lib:
        B = C.CDLL(os.path.abspath(a.baseline_lib))
        for name in ("fcn8s_op_tf_adam", "fcn8s_op_sgd_momentum", "fcn8s_op_tf_adam_ema", "fcn8s_op_sgd_momentum_ema"):
            getattr(B, name).restype, getattr(B, name).argtypes = L.SIGNATURES[name]
    base = {"tf_adam": (lambda: L.check(B.fcn8s_op_tf_adam(stream(), p(th), p(gr), p(m), p(v), n, 1000, lr, 0.9, 0.999, 1e-8, 1.0)),
                        lambda: L.check(B.fcn8s_op_tf_adam_ema(stream(), p(th), p(gr), p(m), p(v), p(s), n, 1000, lr, 0.9, 0.999, 1e-8, 1.0, None, w))),
            "sgd_momentum": (lambda: L.check(B.fcn8s_op_sgd_momentum(stream(), p(th), p(gr), p(m), n, lr, 0.9, 1.0)),
                             lambda: L.check(B.fcn8s_op_sgd_momentum_ema(stream(), p(th), p(gr), p(m), p(s), n, lr, 0.9, 1.0, None, w)))}
    held = True

    def then(f1, f2):
        def run():
            f1(); f2()
        return run

    for name, off, fused, b_off, b_fused in (("tf_adam", adam_off, adam_fused, 28, 36), ("sgd_momentum", sgd_off, sgd_fused, 20, 28)):
        cands = {"off": off, "fused": fused, "unfused": then(off, ema)}
        if B:
            cands.update(baseline_off=base[name][0], baseline_fused=base[name][1])
        r = alternate(cands, a.reps, a.rounds)
        fo, uo, fu = ratio_spread(r["fused"], r["off"]), ratio_spread(r["unfused"], r["off"]), ratio_spread(r["fused"], r["unfused"])
        emit(dict(kind="update", optimizer=name, elements=n, off=stats(r["off"]), fused=stats(r["fused"]), unfused=stats(r["unfused"]),
                  fused_over_off=fo, unfused_over_off=uo, fused_over_unfused=fu,
                  estimate_fused_over_off=round(b_fused / b_off, 3), estimate_unfused_over_off=round((b_off + 12) / b_off, 3),
                  fused_faster=bool(np.median(r["fused"]) < np.median(r["unfused"])),
                  fused_tbps=round(b_fused * n / float(np.median(r["fused"])) / 1e9, 3), off_tbps=round(b_off * n / float(np.median(r["off"])) / 1e9, 3),
                  rounds=a.rounds, reps=a.reps))
        for leg in ("off", "fused") if B else ():
            bl = r["baseline_" + leg]
            spread = float(np.max(bl) - np.min(bl))
            ok = bool(np.median(r[leg]) <= np.median(bl) + spread)
            held = held and ok
            emit(dict(kind="vs_baseline", optimizer=name, average=leg == "fused", this=stats(r[leg]), baseline=stats(bl),
                      baseline_spread_ms=round(spread, 4), this_over_baseline=ratio_spread(r[leg], bl), no_slower=ok, rounds=a.rounds, reps=a.reps))
    if B:      # one step of either library from identical inputs (slots and shadow that are not zero, a step that moves theta): the same bits
        m.copy_(torch.randn(n, device="cuda", generator=g) * 0.1); v.copy_(torch.randn(n, device="cuda", generator=g) ** 2)
        s.copy_(th * 1.0001)
        for name in ("tf_adam", "sgd_momentum"):
            for leg in ("off", "fused"):
                got = []
                for lib in (L.lib, B):
                    x = [t.clone() for t in (th, m, v, s)]
                    if name == "tf_adam" and leg == "off":
                        rc = lib.fcn8s_op_tf_adam(stream(), p(x[0]), p(gr), p(x[1]), p(x[2]), n, 3, 1e-3, 0.9, 0.999, 1e-8, 0.37)
                    elif name == "tf_adam":
                        rc = lib.fcn8s_op_tf_adam_ema(stream(), p(x[0]), p(gr), p(x[1]), p(x[2]), p(x[3]), n, 3, 1e-3, 0.9, 0.999, 1e-8, 0.37, None, w)
                    elif leg == "off":
                        rc = lib.fcn8s_op_sgd_momentum(stream(), p(x[0]), p(gr), p(x[1]), n, 1e-2, 0.9, 0.37)
                    else:
                        rc = lib.fcn8s_op_sgd_momentum_ema(stream(), p(x[0]), p(gr), p(x[1]), p(x[3]), n, 1e-2, 0.9, 0.37, None, w)
                    L.check(rc)
                    torch.cuda.synchronize()
                    got.append(x)
                eq = {k: bool(torch.equal(got[0][i].view(torch.int32), got[1][i].view(torch.int32))) for i, k in enumerate(("theta", "m", "v", "s"))}
                moved = not torch.equal(got[0][0], th)
                held = held and all(eq.values()) and moved
                emit(dict(kind="bits_vs_baseline", optimizer=name, average=leg == "fused", elements=n, equal=eq, theta_moved=moved))
                del got, x
    r = alternate({"swap": lambda: L.check(L.lib.fcn8s_op_swap(stream(), p(th), p(s), n)),
                   "ema_update": ema}, a.reps - a.reps % 2 or 2, a.rounds)          # (an even number of swaps: theta is back where it was)
    emit(dict(kind="kernel", name="swap", elements=n, bytes=16 * n, swap=stats(r["swap"]), tbps=round(16 * n / float(np.median(r["swap"])) / 1e9, 3),
              ema_update=stats(r["ema_update"]), ema_update_tbps=round(12 * n / float(np.median(r["ema_update"])) / 1e9, 3), rounds=a.rounds))
    del m, v, s
    e.close()
    del e
    torch.cuda.empty_cache()

    if not a.no_step:
        Nb, Hh, Ww = a.batch, a.height, a.width
        e = Engine(NC, widths=widths, device_id=0, seed=0)
        e.init_params(0)
        img = torch.randint(0, 256, (Nb, Hh, Ww, 3), dtype=torch.uint8, device="cuda", generator=g)
        lab = torch.randint(0, NC, (Nb, Hh, Ww), dtype=torch.uint8, device="cuda", generator=g)
        e.set_ema(0.999); e.set_ema(None)         # the shadow exists in both legs: only the update's kernel differs

        def step(decay):
            def run():
                if (e.ema_config or {}).get("decay") != decay:
                    e.set_ema(decay)
                e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False)
            return run
        r = alternate({"ema_off": step(None), "ema_on": step(0.999)}, a.steps, a.step_rounds)
        d = np.asarray(r["ema_on"]) - np.asarray(r["ema_off"])
        emit(dict(kind="step", precision="fp32", batch="%dx%dx%d" % (Nb, Ww, Hh), ema_off=stats(r["ema_off"]), ema_on=stats(r["ema_on"]),
                  added_ms=dict(median=round(float(np.median(d)), 4), min=round(float(np.min(d)), 4), max=round(float(np.max(d)), 4)),
                  on_over_off=ratio_spread(r["ema_on"], r["ema_off"]), estimate_added_ms=round(8.0 * e.flat_params.numel() / 4.7e9, 3),
                  rounds=a.step_rounds, steps_per_round=a.steps))
        e.close()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    if not held:
        raise SystemExit("ema_bench.py: a comparison with --baseline-lib does not hold (rows vs_baseline / bits_vs_baseline)")


if __name__ == "__main__":
    main()
