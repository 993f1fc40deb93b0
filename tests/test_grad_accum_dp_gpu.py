"""Gradient accumulation and the global-norm clip under the library's own communicator with two ranks on one GPU (the shared-memory
stand-in for librccl of tests/test_fake_rccl_gpu.py; tests/fake_rccl/accum_worker.py is one rank): each rank accumulates two
micro-batches of one image per update and steps with a clip that bites.

Reference: one process stepping on all four images with the same clip, to the bar
tests/test_fake_rccl_gpu.py::test_two_native_ranks_step_equals_big_batch_step holds the plain two-rank split to."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "fake_rccl")
FAKE = os.path.join(FAKE_DIR, "librccl.so.1")
from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)

SMALL = (8, 16, 32, 64, 64, 128, 128)


def test_two_ranks_accumulate_clip_and_stay_identical(tmp_path):
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd import optim
    from tests.test_facade_gpu import gen
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(os.path.join(FAKE_DIR, "fake_rccl.c")):
        subprocess.check_call(["make", "-C", FAKE_DIR])
    # one process on all four images: the norm of its first gradient sets a clip that bites (half of it), then two clipped SGD updates
    P = orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = next(gen(4, 32, 64, 4, onehot=False))
    e = Engine(20, widths=SMALL, seed=7); e.set_params(P)
    before = e.flat_params.cpu().numpy().copy()
    e.forward_backward(img, lab, keep_prob=1.0, l2_rate=1e-3)
    max_norm = 0.5 * float(optim.global_norm(e.flat_grads.cpu().numpy()))
    assert max_norm > 0
    e.set_grad_clip(max_norm)
    refs, ref_stats = [], []
    for _ in range(2):
        e.train_step(img, lab, 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        refs.append(e.flat_params.cpu().numpy().copy()); ref_stats.append(e.update_stats())
    e.close()
    assert ref_stats[0]["clip_coef"] < 0.6

    idfile = str(tmp_path / "id.bin")
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env["FCN8S_RCCL_LIBRARY"] = FAKE
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        out = str(tmp_path / ("out%d.json" % r))
        procs.append((subprocess.Popen([sys.executable, os.path.join(FAKE_DIR, "accum_worker.py"), str(r), "2", idfile, out, repr(max_norm)],
                                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out))
    res = []
    t0 = time.time()
    try:
        for p, out in procs:
            text, _ = p.communicate(timeout=max(1.0, 300 - (time.time() - t0)))
            assert p.returncode == 0, text[-3000:]
            res.append(json.load(open(out)))
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
    z0, z1 = np.load(str(tmp_path / "out0.json.npz")), np.load(str(tmp_path / "out1.json.npz"))
    # the replicas stay bit-identical, and so do the clip's numbers
    np.testing.assert_array_equal(z0["params1"], z1["params1"])
    np.testing.assert_array_equal(z0["params2"], z1["params2"])
    for u in range(2):
        a, b = res[0]["updates"][u], res[1]["updates"][u]
        assert a["stats_bits"] == b["stats_bits"], (a, b)
        for r in (a, b):
            # exactly one all-reduce per bucket per update, on the last micro-batch, in backward-production order
            assert r["allreduces_in_fold"] == 0 and r["allreduces"] == list(range(res[0]["num_buckets"])), r
            assert r["step"] == u + 1 and r["pending"] == 0 and r["skipped"] == 0 and np.isfinite(r["loss"]), r
            assert r["clip_coef"] < (0.6 if u == 0 else 1.0 + 1e-9), r       # the first update's max_norm is half its norm: the clip bites
        assert abs(a["norm"] - ref_stats[u]["norm"]) <= 2e-3 * ref_stats[u]["norm"], (a, ref_stats[u])
        assert abs(a["clip_coef"] - ref_stats[u]["clip_coef"]) <= 2e-3, (a, ref_stats[u])
    # the clipped SGD updates are the big batch's
    for got, ref, prev in ((z0["params1"], refs[0], before), (z0["params2"], refs[1], before)):
        upd_ref, upd = ref - prev, got - prev
        assert np.abs(upd_ref).max() > 0
        err = np.abs(upd - upd_ref).max() / np.abs(upd_ref).max()
        print("2 ranks x 2 micro-batches vs one process on 4 images, clipped: %.3g of the largest update entry" % err)
        assert err <= 2e-3, err
