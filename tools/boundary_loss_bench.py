#!/usr/bin/env python3
"""The kernels of the boundary-weighted cross-entropy: fcn8s_op_boundary_distance next to fcn8s_op_boundary_pair, and the weighted
cross-entropy with and without the table (fcn8s_op_softmax_xent_px / _ex).

Distance leg, per shape (16 x 1024x512, 4 x 2048x1024) and per R in {3, 8, 15}, on the Cityscapes-like label maps of
tools/cityscapes_eval_bench.py:
  * distance_us: fcn8s_op_boundary_distance, device events around --reps launches per block, --blocks blocks alternating with
  * pair_us: fcn8s_op_boundary_pair on the same maps (and a damaged prediction) in the same process.  The distance kernel does a strict
    subset of that kernel's work (one map, no contour matching, no histograms): ratio_distance_over_pair above 1 is a defect.
  Each kernel has its own rotation of input sets (rolled copies), sized by what that kernel touches per launch -- 2 bytes per pixel for the
  distance kernel (labels in, codes out), 9 for the pair kernel -- so that the sets of one rotation hold more than 2 x the 256 MiB
  Infinity Cache; each rotation keeps its place across warm-up, blocks and radii, so a set comes round again only after all the others.
  bytes the algorithm needs (1 in + 1 out per pixel) / time.
Loss leg, 16 x 1024x512 x 20 classes, plain layout, class weights: fcn8s_op_softmax_xent_ex against fcn8s_op_softmax_xent_px with the codes
of the batch's labels at R = 8 and a Gaussian table, alternating single calls, device events.  The logits alone (671 MB) are more than
2 x the cache, so every call streams them from HBM.  Both ops allocate their few KB of scratch and synchronise per call: the same overhead
on both sides, included in both figures.
Step leg, 16 x 1024x512, the full-width model in fp32: Engine.train_step on device tensors (labels = the train ids of the same maps) with
the weighting off and on (Engine.set_boundary_loss, R = 8, the loss leg's table), the two states alternating in blocks of --step-reps
steps in one process, every step between two device events.  Per state: the median over its steps and the spread (max - min) of its block
medians.  The condition row records added = on - off against what the step adds, measured in this same run: the distance kernel at this
shape and R (distance leg) plus the table's cost in the loss kernel (loss leg, with - without), plus the off state's own spread --
added_within_kernels_plus_noise; nothing is tuned to make it true.
Prints one JSON line per record, writes them to --out if given and appends the step leg's records to --append-step if given."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cityscapes_eval_bench import CACHE_BYTES, PEAK_HBM, SHAPES, make_maps, timed  # noqa: E402

RADII = (3, 8, 15)


class Rotation:
    """fn(set index) over `nsets` sets, the index running on from call to call"""
    def __init__(self, fn, nsets):
        self.fn, self.nsets, self.i = fn, nsets, 0

    def __call__(self, _unused=None):
        self.fn(self.i % self.nsets)
        self.i += 1


def sets_beyond_cache(bytes_per_set):
    return max(2, -(-2 * CACHE_BYTES // bytes_per_set) + 1)


def kernel_leg(warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    out = []
    for name, n, h, w in SHAPES[:2]:
        gt, _, train = make_maps(n, h, w, "cityscapes_like", seed=n + h)
        P = h * w
        nd, npair = sets_beyond_cache(2 * n * P), sets_beyond_cache(9 * n * P)     # 33 sets of 16 MiB, 9 sets of 72 MiB at both shapes
        assert nd * 2 * n * P > 2 * CACHE_BYTES and npair * 9 * n * P > 2 * CACHE_BYTES
        g0, p0 = torch.from_numpy(gt).cuda().view(n, h, w), torch.from_numpy(train).cuda().view(n, h, w)
        roll = lambda t, k: torch.roll(t, (k * 37, k * 4099), (1, 2)).contiguous()   # the same statistics in distinct memory
        labels = [roll(g0, k) for k in range(nd)]
        codes = [torch.empty((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(nd)]
        preds = [roll(p0, k) for k in range(npair)]
        rings = torch.zeros(17 * 34 * 34, dtype=torch.int64, device="cuda")
        bprec = torch.zeros(18 * 34, dtype=torch.int64, device="cuda"); brec = torch.zeros_like(bprec)
        bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        for R in RADII:
            distance = Rotation(lambda k: L.check(lib.fcn8s_op_boundary_distance(None, ptr(labels[k]), n, h, w, R, ptr(codes[k]))), nd)
            pair = Rotation(lambda k: L.check(lib.fcn8s_op_boundary_pair(None, ptr(labels[k]), ptr(preds[k]), 0, n, h, w, R, ptr(rings), ptr(bprec),
                                                                        ptr(brec), ptr(bad))), npair)
            td, tp = [], []
            for _ in range(blocks):                                    # alternating blocks: both see the same clocks and neighbours
                td.append(timed(distance, 1, warmup, reps)); tp.append(timed(pair, 1, warmup, reps))
            torch.cuda.synchronize()
            near = float((codes[0] != 255).float().mean())
            d_us, p_us = float(np.median(td)), float(np.median(tp))
            rec = dict(leg="distance", shape=name, maps="cityscapes_like", R=R, distance_sets=nd, pair_sets=npair, reps=reps, blocks=blocks,
                       pixels_within_R_of_a_boundary=round(near, 4),
                       distance_us=round(d_us, 2), distance_us_min=round(min(td), 2), distance_us_max=round(max(td), 2),
                       pair_us=round(p_us, 2), pair_us_min=round(min(tp), 2), pair_us_max=round(max(tp), 2),
                       ratio_distance_over_pair=round(d_us / p_us, 3), bytes_needed=2 * n * P,
                       distance_TBps=round(2 * n * P / d_us * 1e-6, 3), fraction_of_hbm_8TBps=round(2 * n * P / (d_us * 1e-6) / PEAK_HBM, 4))
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del labels, codes, preds
        torch.cuda.empty_cache()
    return out


def loss_leg(reps, warmup):
    import torch
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    from fcn8s_tensorflow_amd import loss as LM
    lib = L.lib
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    name, n, h, w = SHAPES[0]
    NC, R = 20, 8
    npix = n * h * w
    gt, _, _ = make_maps(n, h, w, "cityscapes_like", seed=5)
    lut = np.full(256, 255, np.uint8)                                  # label ids -> the 20 train ids, 255 (ignore) elsewhere
    lut[ce.TRAINIDS_TO_IDS_ARRAY] = np.arange(len(ce.TRAINIDS_TO_IDS_ARRAY), dtype=np.uint8)
    lab = torch.from_numpy(lut[gt].reshape(n, h, w)).cuda()
    codes = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    L.check(lib.fcn8s_op_boundary_distance(None, ptr(lab), n, h, w, R, ptr(codes)))
    g = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn((npix, NC), device="cuda", generator=g) * 3
    dl = torch.empty_like(logits); lo = torch.zeros(1, device="cuda")
    cw = torch.linspace(0.5, 2.0, NC, device="cuda")
    tab = torch.from_numpy(LM.boundary_table(10.0, 5.0, R)).cuda()

    def ex():
        L.check(lib.fcn8s_op_softmax_xent_ex(None, ptr(logits), ptr(lab), ptr(cw), 0.0, 0, ptr(dl), ptr(lo), None, None, npix, NC))

    def px():
        L.check(lib.fcn8s_op_softmax_xent_px(None, ptr(logits), ptr(lab), ptr(cw), 0.0, 0, ptr(codes), ptr(tab), ptr(dl), ptr(lo), None, None, npix, NC))

    def one(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3

    for _ in range(warmup):
        one(ex); one(px)
    te, tx = [], []
    for _ in range(reps):                                              # alternating single calls
        te.append(one(ex)); tx.append(one(px))
    e_us, x_us = float(np.median(te)), float(np.median(tx))
    by = npix * (NC * 4 * 2 + 1)
    rec = dict(leg="loss", shape=name, classes=NC, R=R, table="1 + 10 exp(-d2 / 50)", reps=reps,
               pixels_within_R_of_a_boundary=round(float((codes != 255).float().mean()), 4),
               weighted_us=round(e_us, 2), weighted_us_min_max=[round(min(te), 2), round(max(te), 2)],
               weighted_with_table_us=round(x_us, 2), weighted_with_table_us_min_max=[round(min(tx), 2), round(max(tx), 2)],
               ratio_with_over_without=round(x_us / e_us, 4), bytes_without=by, bytes_with=by + npix,
               weighted_TBps=round(by / e_us * 1e-6, 3), weighted_with_table_TBps=round((by + npix) / x_us * 1e-6, 3))
    print(json.dumps(rec), flush=True)
    return [rec]


def step_leg(kernel_recs, loss_rec, warmup, reps, blocks):
    import torch
    from fcn8s_tensorflow_amd import cityscapes_eval as ce
    from fcn8s_tensorflow_amd import loss as LM
    from fcn8s_tensorflow_amd.engine import Engine
    name, n, h, w = SHAPES[0]
    NC, R = 20, 8
    gt, _, _ = make_maps(n, h, w, "cityscapes_like", seed=5)
    lut = np.full(256, 255, np.uint8)
    lut[ce.TRAINIDS_TO_IDS_ARRAY] = np.arange(len(ce.TRAINIDS_TO_IDS_ARRAY), dtype=np.uint8)
    lab = torch.from_numpy(lut[gt].reshape(n, h, w)).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
    table = LM.boundary_table(10.0, 5.0, R)
    e = Engine(NC, device_id=0, seed=0)
    states = (("off", lambda: e.set_boundary_loss()), ("on", lambda: e.set_boundary_loss(table, R)))

    def run(k):
        """k steps queued back to back, each between two device events of its own -> ms per step"""
        ev = []
        for _ in range(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False); b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    for _, switch in states:                                           # both states' buffers exist before anything is timed
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
    np.testing.assert_array_equal(e.boundary_codes()[0], LM.boundary_codes_numpy(lab[0].cpu().numpy(), R))   # the timed path is the checked one
    e.close()
    out = []
    stat = {}
    for st in ("off", "on"):
        stat[st] = (float(np.median(steps[st])), max(meds[st]) - min(meds[st]))
        out.append(dict(leg="step", state=st, shape=name, precision="fp32", R=R if st == "on" else 0, table="1 + 10 exp(-d2 / 50)" if st == "on" else None,
                        steps_per_block=reps, blocks=blocks, step_ms=round(stat[st][0], 4), block_median_ms_min=round(min(meds[st]), 4),
                        block_median_ms_max=round(max(meds[st]), 4), block_median_spread_ms=round(stat[st][1], 4)))
    d_us = next(r["distance_us"] for r in kernel_recs if r["shape"] == name and r["R"] == R)
    table_us = loss_rec["weighted_with_table_us"] - loss_rec["weighted_us"]
    added = stat["on"][0] - stat["off"][0]
    bound = (d_us + table_us) * 1e-3 + stat["off"][1]
    out.append(dict(leg="step_condition", shape=name, R=R, added_ms=round(added, 4), added_fraction_of_step=round(added / stat["off"][0], 5),
                    t_distance_ms=round(d_us * 1e-3, 4), t_px_minus_ex_ms=round(table_us * 1e-3, 4), spread_off_ms=round(stat["off"][1], 4),
                    bound_ms=round(bound, 4), added_within_kernels_plus_noise=bool(added <= bound)))
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="launches per block")
    ap.add_argument("--blocks", type=int, default=20, help="alternating blocks")
    ap.add_argument("--step-reps", type=int, default=8, help="timed training steps per block of the step leg")
    ap.add_argument("--step-blocks", type=int, default=10, help="alternating blocks per state of the step leg")
    ap.add_argument("--out")
    ap.add_argument("--append-step", help="append the step leg's records to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("boundary_loss_bench.py measures on an MI355X; no GPU here")
    kernels = kernel_leg(a.warmup, a.reps, a.blocks)
    loss = loss_leg(max(20, a.reps), a.warmup)
    torch.cuda.empty_cache()
    steps = step_leg(kernels, loss[0], a.warmup, a.step_reps, a.step_blocks)
    recs = kernels + loss + steps
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    if a.append_step:
        os.makedirs(os.path.dirname(os.path.abspath(a.append_step)), exist_ok=True)
        with open(a.append_step, "a") as f:
            for r in steps:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
