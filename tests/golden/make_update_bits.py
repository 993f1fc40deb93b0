#!/usr/bin/env python
"""Generates tests/golden/update_bits.npz: the bits of one TF-Adam and one SGD-momentum step as a build of the PARENT commit of the change
that made csrc/optim.hip's update kernel the only one computes them on an MI355X -- the hand-vectorised kernels that change retired.  Run
once, on the GPU, against that build; never regenerated from the code under test:

    python tests/golden/make_update_bits.py --lib PARENT_BUILD/fcn8s_tensorflow_amd/libfcn8s_hip.so --commit PARENT_COMMIT_ID

  inputs: tests.test_ema_ops_gpu.make_inputs (the seeded arrays of that test's `data` fixture), copied to 16-byte aligned device buffers;
  fcn8s_op_tf_adam (t = 3, lr 1e-3, 0.9, 0.999, 1e-8, gs = 0.37) and fcn8s_op_sgd_momentum (lr 1e-2, 0.9, gs = 0.37), the calls of that
  test's _reference_update.

Stored per optimizer (adam: theta, m, v; sgd: theta, m) and size n: <opt>_<array>_<n>, float32 [n], for the RAW sizes; for the DIGEST sizes
<opt>_<array>_sha256_<n>, the SHA-256 of the array's bytes as a hex string.  `commit` and `hipcc_version` say what produced them.
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
RAW = (1, 3, 4, 5, 255, 1023, 1025)
DIGEST = (262147, 2098181)
ARRAYS = {"adam": ("theta", "m", "v"), "sgd": ("theta", "m")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libfcn8s_hip.so of the parent commit's build")
    ap.add_argument("--commit", required=True, help="the parent commit's id")
    ap.add_argument("--out", default=os.path.join(HERE, "update_bits.npz"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from tests.test_ema_ops_gpu import make_inputs, ptr
    lib = C.CDLL(os.path.abspath(a.lib))          # (the prototypes of _lib.py, written out: importing it would load this tree's library)
    p, f = C.c_void_p, C.c_float
    lib.fcn8s_op_tf_adam.restype, lib.fcn8s_op_tf_adam.argtypes = C.c_int, [p, p, p, p, p, C.c_int64, C.c_int, f, f, f, f, f]
    lib.fcn8s_op_sgd_momentum.restype, lib.fcn8s_op_sgd_momentum.argtypes = C.c_int, [p, p, p, p, C.c_int64, f, f, f]
    data = make_inputs()
    out = {"commit": np.str_(a.commit),
           "hipcc_version": np.str_(subprocess.check_output([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], text=True).strip())}
    for n in RAW + DIGEST:
        for opt in ("adam", "sgd"):
            t = {k: torch.from_numpy(data[n][k].copy()).cuda() for k in ("theta", "g", "m", "v")}
            assert all(x.data_ptr() % 16 == 0 for x in t.values())
            if opt == "adam":
                rc = lib.fcn8s_op_tf_adam(None, ptr(t["theta"]), ptr(t["g"]), ptr(t["m"]), ptr(t["v"]), n, 3, 1e-3, 0.9, 0.999, 1e-8, 0.37)
            else:
                rc = lib.fcn8s_op_sgd_momentum(None, ptr(t["theta"]), ptr(t["g"]), ptr(t["m"]), n, 1e-2, 0.9, 0.37)
            assert rc == 0, (opt, n, rc)
            torch.cuda.synchronize()
            for k in ARRAYS[opt]:
                got = t[k].cpu().numpy()
                if n in RAW:
                    out["%s_%s_%d" % (opt, k, n)] = got
                else:
                    out["%s_%s_sha256_%d" % (opt, k, n)] = np.str_(hashlib.sha256(got.tobytes()).hexdigest())
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
