"""One rank of tests/test_grad_accum_dp_gpu.py: like worker.py a process of its own on GPU 0 over the shared-memory stand-in for librccl,
here accumulating two micro-batches of one image per update and stepping with the global-norm clip on.

    python tests/fake_rccl/accum_worker.py <rank> <world> <id file> <out file> <max_norm>
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.fake_rccl.worker import SMALL, unique_id  # noqa: E402


def main():
    rank, world, idfile, outfile, max_norm = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], float(sys.argv[5])
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    from oracle import fcn8s_oracle as orc      # checker only: the synthetic parameters of the other GPU tests
    from tests.test_facade_gpu import gen
    e = Engine(20, widths=SMALL, device_id=0, seed=7)
    P = orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05)
    if rank != 0:                               # rank 0's parameters arrive through the broadcast
        P = {k: np.zeros_like(v) for k, v in P.items()}
    e.set_params(P)
    img, lab = next(gen(2 * world, 32, 64, 4, onehot=False))
    e.comm_init_native(unique_id(L, rank, idfile), rank, world)
    e.broadcast_params(0)
    e.set_grad_clip(max_norm)

    # every all-reduce the engine asks the library for goes through this counter (one ncclAllReduce each: fcn8s_allreduce_bucket)
    calls = []
    real = L.lib.fcn8s_allreduce_bucket
    L.lib.fcn8s_allreduce_bucket = lambda h, b: (calls.append(int(b)), real(h, b))[1]

    res = {"rank": rank, "num_buckets": e.num_buckets, "updates": []}
    for u in range(2):
        n0 = len(calls)
        e.accumulate_step(img[2 * rank:2 * rank + 1], lab[2 * rank:2 * rank + 1], keep_prob=1.0, l2_rate=1e-3)
        after_fold = len(calls) - n0
        loss, step = e.train_step(img[2 * rank + 1:2 * rank + 2], lab[2 * rank + 1:2 * rank + 2], 1e-2, keep_prob=1.0, l2_rate=1e-3,
                                  optimizer=L.OPT_SGD_MOMENTUM)
        st = e.update_stats()
        res["updates"].append(dict(allreduces_in_fold=after_fold, allreduces=calls[n0:], step=step, loss=loss, pending=e.pending_micro_batches,
                                   skipped=st["skipped"],
                                   stats_bits=[int(np.float32(st[k]).view(np.uint32)) for k in ("norm", "clip_coef", "scale")],
                                   clip_coef=st["clip_coef"], norm=st["norm"]))
        if u == 0:
            params1 = e.flat_params.cpu().numpy().copy()
    np.savez(outfile + ".npz", params1=params1, params2=e.flat_params.cpu().numpy())
    L.lib.fcn8s_allreduce_bucket = real
    e.comm_destroy()
    e.close()
    json.dump(res, open(outfile, "w"))


if __name__ == "__main__":
    main()
