#!/usr/bin/env python3
"""The focal loss (fcn8s_set_focal, fcn8s_op_focal_xent): its kernel against a copy of its bytes and against the cross-entropy op on the same
inputs, and what it adds to the training step.

Op leg, per shape (16 x 1024x512 x 20, 1 x 2048x1024 x 20), without and with class weights + distance codes: fcn8s_op_focal_xent on the plain layout
-- the model's kernel and reduction, gamma = 2 -- between two device events around --reps back-to-back calls, its inputs (logits, labels, codes)
and its dlogits rotated through sets that together exceed 2 x the 256 MiB Infinity Cache.  Alternating with it in blocks in the same process:
  - a device-to-device copy of the kernel's algorithmic bytes ((8 C + 1 or 2) per pixel: logits 4 C, dlogits 4 C, the label byte, the code byte), half
    of them read and half written, rotated the same way; ratio_to_copy against the 1.25 x the project's streaming kernels aim at;
  - fcn8s_op_softmax_xent_px on the same inputs (the plain mean without weights, the weighted mode with them): it moves the same bytes, so
    focal_minus_xent_us against that op's own block spread (max - min of its block means) is the second row.
Both are reported, not asserted.
Step leg, 16 x 1024x512, full-width fp32: Engine.train_step on device tensors with gamma off (nothing of the focal loss is launched: the parent
commit's step) and on, the two states alternating in blocks of --step-reps steps, every step between two device events.  Per state the median over
its steps and the spread (max - min) of its block medians.  The condition row: added = on - off against t(focal_xent group) - t(softmax_xent group),
each measured per step in a block of its own after the timed ones, plus the off state's spread; nothing is tuned to make it true.
Prints one JSON line per record and writes them to --out if given."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, timed  # noqa: E402

SHAPES = [("16x1024x512", 16, 512, 1024), ("1x2048x1024", 1, 1024, 2048)]
NC, BAR, GAMMA = 20, 1.25, 2.0


def op_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    out = []
    nwork = int(L.lib.fcn8s_op_focal_xent_work_bytes())
    work = torch.empty(nwork, dtype=torch.uint8, device="cuda")
    loss = torch.zeros(1, device="cuda")
    xloss = torch.zeros(1, device="cuda")
    bias = torch.zeros(NC, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    cw = (torch.rand(NC, device="cuda", generator=g) + 0.5).contiguous()
    table = (torch.rand(256, device="cuda", generator=g) * 2 + 0.5).contiguous()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for name, n, h, w in SHAPES:
        npix = n * h * w
        for weighted in (False, True):
            by = npix * (8 * NC + (2 if weighted else 1))
            half = by // 2 // 16 * 16
            nsets = max(2, -(-2 * CACHE_BYTES // by) + 1)
            zs = [torch.randn((npix, NC), device="cuda", generator=g).mul_(3.0) for _ in range(nsets)]
            ds = [torch.zeros((npix, NC), device="cuda") for _ in range(nsets)]
            src = [torch.empty(half, dtype=torch.uint8, device="cuda").random_() for _ in range(nsets)]
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            labs, codes = [], []
            for _ in range(nsets):
                lab = torch.randint(0, NC, (npix,), dtype=torch.uint8, device="cuda", generator=g)
                lab[torch.rand(npix, device="cuda", generator=g) < 0.05] = 255
                labs.append(lab)
                codes.append(torch.randint(0, 256, (npix,), dtype=torch.uint8, device="cuda", generator=g) if weighted else None)
            a_cw, a_tab = (cw, table) if weighted else (None, None)
            copy = lambda k: dst.copy_(src[k % nsets])

            def focal(k):
                k %= nsets
                L.check(L.lib.fcn8s_op_focal_xent(None, p(zs[k]), p(labs[k]), p(a_cw), p(codes[k]), p(a_tab), GAMMA, p(ds[k]), p(loss), p(bias), npix, NC,
                                                  p(work), nwork))

            def xent(k):
                k %= nsets
                L.check(L.lib.fcn8s_op_softmax_xent_px(None, p(zs[k]), p(labs[k]), p(a_cw), 0.0, 0, p(codes[k]), p(a_tab), p(ds[k]), p(xloss), None, None,
                                                       npix, NC))
            tk, tx, tc = [], [], []
            for _ in range(blocks):                                    # alternating blocks: all three see the same clocks and neighbours
                tk.append(timed(focal, nsets, warmup, reps))
                tx.append(timed(xent, nsets, warmup, reps))
                tc.append(timed(copy, nsets, warmup, reps))
            k_us, x_us, c_us = float(np.median(tk)), float(np.median(tx)), float(np.median(tc))
            x_spread = max(tx) - min(tx)
            rec = dict(leg="op", shape=name, classes=NC, layout="plain", gamma=GAMMA, weights_and_codes=weighted, reps=reps, blocks=blocks, input_sets=nsets,
                       bytes_needed=by, bytes_per_pixel=by / npix,
                       kernel_us=round(k_us, 2), kernel_us_min_max=[round(min(tk), 2), round(max(tk), 2)],
                       xent_us=round(x_us, 2), xent_us_min_max=[round(min(tx), 2), round(max(tx), 2)], xent_block_spread_us=round(x_spread, 2),
                       copy_us=round(c_us, 2), copy_us_min_max=[round(min(tc), 2), round(max(tc), 2)], copy_bytes=2 * half,
                       ratio_to_copy=round(k_us / c_us, 3), within_bar=bool(k_us / c_us <= BAR), bar=BAR,
                       ratio_to_xent=round(k_us / x_us, 3), focal_minus_xent_us=round(k_us - x_us, 2), within_xent_spread=bool(k_us - x_us <= x_spread),
                       kernel_TBps=round(by / k_us * 1e-6, 3), fraction_of_hbm_8TBps=round(by / (k_us * 1e-6) / PEAK_HBM, 4),
                       loss=float(loss.cpu()[0]), xent_loss=float(xloss.cpu()[0]))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del zs, ds, src, dst, labs, codes
            torch.cuda.empty_cache()
    return out


def step_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    name, n, h, w = SHAPES[0]
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    lab = torch.randint(0, NC, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    lab[torch.rand((n, h, w), device="cuda", generator=g) < 0.05] = 255
    e = Engine(NC, device_id=0, seed=0)
    layout = "blocked" if e.get_option("tconv_gemm") else "plain"
    states = (("off", lambda: e.set_focal()), ("on", lambda: e.set_focal(GAMMA)))

    def run(k):
        """k steps queued back to back, each between two device events of its own -> ms per step"""
        ev = []
        for _ in range(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False)
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    for st, switch in states:                                          # both states' buffers exist before anything is timed
        switch()
        run(max(2, warmup))
    allocs = e.get_option("workspace_allocations")
    steps = {"off": [], "on": []}
    meds = {"off": [], "on": []}
    for _ in range(blocks):                                            # alternating blocks: both states see the same clocks and neighbours
        for st, switch in states:
            switch()
            t = run(reps + 1)[1:]                                      # (the first step behind a switch is not counted)
            steps[st] += t; meds[st].append(float(np.median(t)))
    assert e.get_option("workspace_allocations") == allocs
    grp_us = {}
    for st, switch, group in (("off", states[0][1], "softmax_xent"), ("on", states[1][1], "focal_xent")):    # the loss group's own time per step
        switch()
        e.profile(True); e.profile_reset()
        run(reps)
        grp = e.profile_results()[group]
        assert grp["launches"] == reps
        grp_us[st] = grp["ms"] * 1e3 / reps
        e.profile(False)
    e.close()
    out, stat = [], {}
    for st in ("off", "on"):
        stat[st] = (float(np.median(steps[st])), max(meds[st]) - min(meds[st]))
        out.append(dict(leg="step", state=st, shape=name, precision="fp32", layout=layout, gamma=GAMMA if st == "on" else 0.0,
                        steps_per_block=reps, blocks=blocks, step_ms=round(stat[st][0], 4),
                        block_median_ms_min=round(min(meds[st]), 4), block_median_ms_max=round(max(meds[st]), 4),
                        block_median_spread_ms=round(stat[st][1], 4), loss_group_us=round(grp_us[st], 2)))
    added = stat["on"][0] - stat["off"][0]
    bound = (grp_us["on"] - grp_us["off"]) * 1e-3 + stat["off"][1]
    out.append(dict(leg="step_condition", shape=name, layout=layout, added_ms=round(added, 4), added_fraction_of_step=round(added / stat["off"][0], 5),
                    t_focal_group_ms=round(grp_us["on"] * 1e-3, 4), t_xent_group_ms=round(grp_us["off"] * 1e-3, 4), spread_off_ms=round(stat["off"][1], 4),
                    bound_ms=round(bound, 4), added_within_kernel_difference_plus_noise=bool(added <= bound)))
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="calls (and copies) per block of the op leg")
    ap.add_argument("--blocks", type=int, default=6, help="alternating blocks of the op leg")
    ap.add_argument("--step-reps", type=int, default=8, help="timed training steps per block of the step leg")
    ap.add_argument("--step-blocks", type=int, default=8, help="alternating blocks per state of the step leg")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("focal_bench.py measures on an MI355X; no GPU here")
    recs = op_leg(a.warmup, a.reps, a.blocks)
    torch.cuda.empty_cache()
    if not a.skip_step:
        recs += step_leg(a.warmup, a.step_reps, a.step_blocks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
