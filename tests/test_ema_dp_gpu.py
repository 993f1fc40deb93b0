"""The parameter average under the library's own communicator with two ranks on one GPU (the shared-memory stand-in for librccl of
tests/test_fake_rccl_gpu.py; tests/fake_rccl/ema_worker.py is one rank): one 64x64 image per rank, two SGD-momentum updates, the
average on.  Nothing is exchanged for the shadow: the replicas hold identical parameters, so they hold identical shadows.

References: the other rank (bits); optim.py's float64 recursion over a rank's own parameter snapshots (4 K 2^-23 M, K = 2); one process
stepping on both images.  The two-rank parameters equal the one-process parameters only up to fp32 summation order (the bar of
tests/test_fake_rccl_gpu.py::test_two_native_ranks_step_equals_big_batch_step: 2e-3 of the largest update entry), and the shadow is a
linear function of the snapshots with the same coefficients in both runs.  So the shadows are compared after taking out what the
parameters' own difference contributes: |(s_rank - s_one) - R(theta_rank - theta_one)| <= 2 * 4 K 2^-23 M, R the recursion -- one bound
for each run's rounding.  A rank that averaged with another weight, another step number or other parameters fails it."""
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


def test_two_ranks_hold_the_same_shadow_and_it_is_the_big_batch_one(tmp_path):
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    from fcn8s_tensorflow_amd import optim
    from tests.fake_rccl.ema_worker import DECAY, STEPS, batch
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(os.path.join(FAKE_DIR, "fake_rccl.c")):
        subprocess.check_call(["make", "-C", FAKE_DIR])
    # one process on both images
    img, lab = batch(2)
    e = Engine(20, widths=SMALL, seed=7)
    e.set_params(orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05))
    e.set_ema(DECAY)
    s0 = e.get_ema()
    one = []
    for _ in range(STEPS):
        e.train_step(img, lab, 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
        one.append(e.flat_params.cpu().numpy().copy())
    s_one = e.get_ema()
    e.close()

    idfile = str(tmp_path / "id.bin")
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env["FCN8S_RCCL_LIBRARY"] = FAKE
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        out = str(tmp_path / ("out%d.json" % r))
        procs.append((subprocess.Popen([sys.executable, os.path.join(FAKE_DIR, "ema_worker.py"), str(r), "2", idfile, out],
                                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out))
    t0 = time.time()
    try:
        for p, out in procs:
            text, _ = p.communicate(timeout=max(1.0, 300 - (time.time() - t0)))
            assert p.returncode == 0, text[-3000:]
            assert json.load(open(out))["steps"] == list(range(1, STEPS + 1))
    finally:
        for p, _ in procs:
            if p.poll() is None:
                p.kill()
    z = [np.load(str(tmp_path / ("out%d.json.npz" % r))) for r in range(2)]
    # the replicas: identical parameters, identical shadows, bit for bit
    for key in ["shadow0", "shadow"] + ["params%d" % (u + 1) for u in range(STEPS)]:
        assert z[0][key].tobytes() == z[1][key].tobytes(), key
    assert z[0]["shadow0"].tobytes() == s0.tobytes()                      # the shadow starts from the broadcast parameters
    assert z[0]["shadow"].tobytes() != z[0]["params%d" % STEPS].tobytes() != s0.tobytes()

    def recursion(start, thetas):
        s = np.asarray(start, np.float64)
        for t, th in enumerate(thetas, 1):
            s = optim.ema_step(s, th, optim.ema_omega(DECAY, t, True))
        return s

    for r in range(2):
        snaps = [z[r]["params%d" % (u + 1)] for u in range(STEPS)]
        M = np.max(np.abs(np.stack([s0] + snaps + one)), axis=0).astype(np.float64)
        bound = 4.0 * STEPS * 2.0 ** -23 * M
        got = z[r]["shadow"].astype(np.float64)
        # the definition, over the rank's own snapshots
        assert (np.abs(got - recursion(s0, snaps)) <= bound).all()
        # the one-process shadow, the parameters' own summation-order difference taken out (module docstring)
        carried = recursion(np.zeros_like(got), [a.astype(np.float64) - b.astype(np.float64) for a, b in zip(snaps, one)])
        resid = np.abs((got - s_one.astype(np.float64)) - carried)
        print("rank %d: shadow vs one process: %.3g of 2 x the bound; raw difference %.3g of the largest shadow movement"
              % (r, float((resid / np.maximum(2 * bound, 1e-300)).max()),
                 float(np.abs(got - s_one).max() / np.abs(s_one.astype(np.float64) - s0).max())))
        assert (resid <= 2 * bound).all()
        # ... and with it: as close as the parameters themselves are
        assert np.abs(got - s_one).max() <= 2e-3 * np.abs(s_one.astype(np.float64) - s0).max()
