#!/usr/bin/env python3
"""The training loss modes (fcn8s_set_loss) at 16 x 1024x512, fp32, full width: default (the reference's mean), class-weighted, and OHEM
(thresh 0.7, min_kept 100 000) with the same weights, and OHEM with min_kept deciding the threshold (thresh 1e-30).

Per mode, on one engine whose loss configuration is switched between the modes:
  * ms per TF-Adam training step (device inputs, synchronised, median of --steps steps after --warmup);
  * the softmax_xent profile group (every loss kernel of the mode, ms per step and its algorithmic bytes / ms) in a separate profiled
    run, and the loss statistics |V|, |K| and t of the last step;
  * workspace_allocations before and after the timed steps.
The labels are uniform over the 20 classes with about 5 % ignore ids, so OHEM's min_kept or tau decides as the random model's losses do.
Prints one JSON line per mode and writes them to --out if given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, NC = 16, 512, 1024, 20
TARGET_MS = {"default": None, "weighted": None, "ohem": 0.6, "ohem_select": 0.6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    e = Engine(NC, device_id=0, seed=0)
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    lab = torch.randint(0, NC, (N, H, W), dtype=torch.uint8, device="cuda", generator=g)
    lab[torch.rand((N, H, W), device="cuda", generator=g) < 0.05] = 255
    cw = np.linspace(0.5, 2.0, NC)
    # "ohem_select": tau = 69 lies above every loss, so min_kept decides t and the radix refinement passes run (in "ohem" a random model's
    # losses, about ln 20, all exceed tau = 0.357: the selection stops after the first histogram)
    modes = [("default", {}), ("weighted", dict(class_weights=cw)), ("ohem", dict(class_weights=cw, ohem_thresh=0.7, ohem_min_kept=100000)),
             ("ohem_select", dict(class_weights=cw, ohem_thresh=1e-30, ohem_min_kept=100000))]
    rows = []
    for name, cfg in modes:
        e.set_loss(**cfg)
        step = lambda: e.train_step(img, lab, 1e-6, keep_prob=0.5, fetch_loss=False)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        a0 = e.get_option("workspace_allocations")
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        a1 = e.get_option("workspace_allocations")
        e.profile(True); e.profile_reset()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        r = e.profile_results().get("softmax_xent", dict(ms=0.0, launches=0, bytes=0.0))
        e.profile(False)
        stats = e.loss_stats() if cfg else None
        ms = r["ms"] / 3
        row = dict(mode=name, batch="%dx%dx%d" % (N, W, H), precision="fp32", step_ms_median=round(float(np.median(ts)) * 1e3, 3),
                   step_ms_min=round(float(np.min(ts)) * 1e3, 3), loss_stage_ms=round(ms, 4), loss_stage_launches=r["launches"] // 3,
                   loss_stage_bytes=r["bytes"] / 3, loss_stage_tbps=round(r["bytes"] / 3 / (ms * 1e-3) / 1e12, 3) if ms > 0 else None,
                   loss_stage_target_ms=TARGET_MS[name], loss_stats=stats, workspace_allocations=[a0, a1], config={k: (list(map(float, v)) if k == "class_weights" else v) for k, v in cfg.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    base = rows[0]["loss_stage_ms"]
    summary = dict(mode="summary", weighted_vs_default_loss_stage=round(rows[1]["loss_stage_ms"] / base - 1, 4) if base else None,
                   ohem_vs_default_loss_stage=round(rows[2]["loss_stage_ms"] / base - 1, 4) if base else None,
                   weighted_vs_default_step=round(rows[1]["step_ms_median"] / rows[0]["step_ms_median"] - 1, 4),
                   ohem_vs_default_step=round(rows[2]["step_ms_median"] / rows[0]["step_ms_median"] - 1, 4),
                   ohem_select_vs_default_loss_stage=round(rows[3]["loss_stage_ms"] / base - 1, 4) if base else None,
                   ohem_select_vs_default_step=round(rows[3]["step_ms_median"] / rows[0]["step_ms_median"] - 1, 4))
    rows.append(summary)
    print(json.dumps(summary), flush=True)
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
