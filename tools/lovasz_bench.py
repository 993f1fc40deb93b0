#!/usr/bin/env python3
"""The Lovász-softmax training loss (fcn8s_set_lovasz) at 16 x 1024x512, 20 classes, full width, in fp32 and bf16_train: off, batch
(one sort per class over the whole batch) and per-image (one sort per image and class).

Per precision and mode, on one engine whose loss configuration is switched between the modes:
  * ms per TF-Adam training step (device inputs, synchronised, median of --steps steps after --warmup);
  * the lovasz profile group (keys, sort, Jaccard scan, gradient; ms per step, algorithmic bytes and the fraction of 8 TB/s) in a
    separate profiled run, and the scratch bytes of the sort;
  * workspace_allocations before and after the timed steps.
The labels are uniform over the 20 classes with about 5 % ignore ids.  Prints one JSON line per row and writes them to --out if given."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, NC = 16, 512, 1024, 20
TARGET_MS = 4.5
HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", default="fp32,bf16_train")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fcn8s_tensorflow_amd.engine import Engine
    rows = []
    for precision in a.precisions.split(","):
        e = Engine(NC, device_id=0, seed=0, precision=precision)
        g = torch.Generator(device="cuda").manual_seed(0)
        img = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        lab = torch.randint(0, NC, (N, H, W), dtype=torch.uint8, device="cuda", generator=g)
        lab[torch.rand((N, H, W), device="cuda", generator=g) < 0.05] = 255
        for name, cfg in (("off", dict(lovasz_weight=0.0)), ("batch", dict(lovasz_weight=0.5)), ("per_image", dict(lovasz_weight=0.5, per_image=True))):
            e.set_lovasz(**cfg)
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
            r = e.profile_results().get("lovasz", dict(ms=0.0, launches=0, bytes=0.0))
            x = e.profile_results().get("softmax_xent", dict(ms=0.0, launches=0, bytes=0.0))
            e.profile(False)
            ms = r["ms"] / 3
            segs = N if cfg.get("per_image") else 1
            L = N * H * W // segs
            tiles = (L + 16383) // 16384
            scratch = 16 * N * H * W * NC + segs * NC * tiles * (1024 * 4 + 12) if cfg["lovasz_weight"] else 0
            row = dict(mode=name, batch="%dx%dx%d" % (N, W, H), classes=NC, precision=precision,
                       step_ms_median=round(float(np.median(ts)) * 1e3, 3), step_ms_min=round(float(np.min(ts)) * 1e3, 3),
                       lovasz_ms=round(ms, 4), lovasz_launches=r["launches"] // 3, lovasz_bytes=r["bytes"] / 3,
                       lovasz_frac_of_8tbps=round(r["bytes"] / 3 / (ms * 1e-3) / HBM, 3) if ms > 0 else None, lovasz_target_ms=TARGET_MS if ms else None,
                       softmax_xent_ms=round(x["ms"] / 3, 4), scratch_bytes=scratch, workspace_allocations=[a0, a1],
                       loss_terms=e.loss_terms(), config=cfg)
            rows.append(row)
            print(json.dumps(row), flush=True)
        e.close()
        del img, lab
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
