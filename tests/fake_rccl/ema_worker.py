"""One rank of tests/test_ema_dp_gpu.py: like worker.py a process of its own on GPU 0 over the shared-memory stand-in for librccl, here
stepping twice with the parameter average on (Engine.set_ema) and writing its parameter snapshots and its shadow.

    python tests/fake_rccl/ema_worker.py <rank> <world> <id file> <out file>
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.fake_rccl.worker import SMALL, unique_id  # noqa: E402

DECAY, STEPS = 0.9, 2


def batch(world):
    rng = np.random.default_rng(17)
    return rng.integers(0, 256, (world, 64, 64, 3), dtype=np.uint8), rng.integers(0, 20, (world, 64, 64), dtype=np.uint8)


def main():
    rank, world, idfile, outfile = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    from oracle import fcn8s_oracle as orc      # checker only: the synthetic parameters of the other GPU tests
    e = Engine(20, widths=SMALL, device_id=0, seed=7)
    P = orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05)
    if rank != 0:                               # rank 0's parameters arrive through the broadcast
        P = {k: np.zeros_like(v) for k, v in P.items()}
    e.set_params(P)
    img, lab = batch(world)
    e.comm_init_native(unique_id(L, rank, idfile), rank, world)
    e.broadcast_params(0)
    e.set_ema(DECAY)                            # behind the broadcast: the shadow starts from rank 0's parameters everywhere
    out = {"shadow0": e.get_ema()}
    steps = []
    for u in range(STEPS):
        _, step = e.train_step(img[rank:rank + 1], lab[rank:rank + 1], 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        steps.append(step)
        out["params%d" % (u + 1)] = e.flat_params.cpu().numpy().copy()
    out["shadow"] = e.get_ema()
    np.savez(outfile + ".npz", **out)
    e.comm_destroy()
    e.close()
    json.dump({"rank": rank, "steps": steps}, open(outfile, "w"))


if __name__ == "__main__":
    main()
