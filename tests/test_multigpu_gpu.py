"""BASELINE config 4 (N x MI355X data-parallel training, gradients all-reduced over RCCL / xGMI): everything that needs a SECOND
GPU.  Every test here is gated on `torch.cuda.device_count() >= 2` and is visibly skipped on a one-GPU box; on such a box the same
code paths run with both ranks on the one GPU over gloo (tests/test_boundary_gpu.py, tests/test_facade_gpu.py) and with one RCCL rank.
The first box with two or more GPUs runs, without any change:

  * `bench.py --gpus N` exactly as the driver launches it (self-launch and under torchrun), over torch.distributed's RCCL backend AND
    over the library's own communicator behind the C ABI (`--comm native`): rccl_ranks == N, four buckets in backward-production order,
    replicas bit-identical after the timed steps;
  * `run_dp.py --gpus N` (FCN8s.train() per rank on its own file shard) over both;
  * a 2-rank RCCL step == the big-batch step (the gloo test of tests/test_facade_gpu.py re-run with one rank per GPU), for both
    communicators -- the native one being the first >1-rank run of fcn8s_comm_* / fcn8s_allreduce_bucket;
  * a rank that dies: the run ends with ONE JSON line carrying an `error` field instead of hanging.

Reference: single-device (fcn8s_tensorflow.py:65); the exchange step is SURVEY 8e's, the loss a mean over N.H.W (:253)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import fcn8s_oracle as orc  # noqa: E402  (checker only)

SMALL = (8, 16, 32, 64, 64, 128, 128)          # tests/test_facade_gpu.py's small network


def _ngpus():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


needs2 = pytest.mark.skipif(_ngpus() < 2, reason="needs >= 2 GPUs (this box has %d): the N-rank RCCL paths run on the first multi-GPU box" % _ngpus())


def _env():
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def _rank_counts():
    n = _ngpus()
    return sorted({2, n} if n >= 2 else {2})


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def _check_dp_line(out, n, comm):
    assert out.get("error") is None, out.get("error")
    assert out["n_gpus"] == n and out["rccl_ranks"] == n and out["config"]["global_batch"] == 2 * n and out["config"]["parallelism"] == "dp%d" % n
    assert len(out["per_rank_ms"]) == n and all(t > 0 for t in out["per_rank_ms"])
    c = out["comm"]
    assert c["backend"] == "nccl" and c["rccl_ranks"] == n and c["ranks"] == n and c["rccl_version"]
    assert c["collectives_by"].startswith("libfcn8s_hip" if comm == "native" else "torch.distributed")
    assert c["replicas_identical_after_timed_steps"] is True
    assert len(c["bucket_mb"]) == len(c["bucket_issue_ms"]) == len(c["bucket_complete_ms"]) == len(c["allreduce_ms_per_bucket_standalone"]) == 4
    assert abs(sum(c["bucket_mb"]) - 537.9) < 1.0 and c["bucket_mb"][1] > 400                      # fc6 alone
    assert c["bucket_issue_ms"] == sorted(c["bucket_issue_ms"])                                    # buckets leave in backward-production order
    assert all(d >= i for i, d in zip(c["bucket_issue_ms"], c["bucket_complete_ms"]))
    assert all(np.isfinite(x) and x > 0 for x in c["allreduce_ms_per_bucket_standalone"])
    assert all(x and x > 0 for x in c["allreduce_busbw_gbs_per_bucket_standalone"])
    assert c["exposed_comm_ms_per_step"] is not None and c["local_only_ms_per_step"] > 0 and isinstance(c["numa"], dict)
    assert out["value"] > 0 and np.isfinite(out["final_loss"]) and out["final_loss_ok"]


@needs2
@pytest.mark.parametrize("comm", ["torch", "native"])
@pytest.mark.parametrize("n", _rank_counts())
def test_bench_n_ranks_over_rccl(n, comm):
    """`python bench.py --gpus N` as the driver calls it (no torchrun: it launches its own ranks), one rank per GPU over RCCL."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "1", "--repeats", "1", "--batch", "2",
                        "--height", "64", "--width", "64", "--no-cpu-baseline", "--full", "--comm", comm], capture_output=True, text=True, timeout=900, env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    _check_dp_line(_json_line(r.stdout), n, comm)


@needs2
def test_bench_under_torchrun_n_ranks_over_rccl():
    """The driver's own N > 1 command line: `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`."""
    import socket
    n = _ngpus()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0)); port = so.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "1", "--repeats", "1",
                        "--batch", "2", "--height", "64", "--width", "64", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=900, env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    _check_dp_line(_json_line(r.stdout), n, "torch")


@needs2
def test_bench_full_size_two_ranks_over_rccl():
    """Config 4's per-GPU shape (16 x 1024x512 per rank) on two ranks: the step with the exchange costs at most 10 % more than the same
    step without it (the budget of DESIGN section 6 is <= 1 ms of 58), and the replicas stay bit-identical."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--repeats", "1", "--no-cpu-baseline", "--full"],
                       capture_output=True, text=True, timeout=1800, env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    out = _json_line(r.stdout)
    c = out["comm"]
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 32 and c["replicas_identical_after_timed_steps"] is True
    print("2 x MI355X, 16 x 1024x512 per rank: %.1f images/s, %.2f ms/step, local-only %.2f ms, exposed %.2f ms" %
          (out["value"], out["ms_per_step"], c["local_only_ms_per_step"], c["exposed_comm_ms_per_step"]))
    assert out["ms_per_step"] <= 1.10 * c["local_only_ms_per_step"], (out["ms_per_step"], c["local_only_ms_per_step"])


@needs2
@pytest.mark.parametrize("comm", ["torch", "native"])
def test_run_dp_n_ranks_over_rccl(comm):
    """run_dp.py (the launcher INTEGRATION.md names): FCN8s.train() on N file shards, gradients and evaluation metrics over RCCL."""
    n = _ngpus()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_dp.py"), "--gpus", str(n), "--comm", comm, "--batch", "2", "--height", "64", "--width", "64",
                        "--steps-per-epoch", "3", "--workers", "0"], capture_output=True, text=True, timeout=900, env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    assert "rank 0: %d ranks x 2 images/step, global step 3" % n in r.stdout, r.stdout[-1000:]


def _rccl_worker(rank, world, port, native, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))     # one rank per GPU: RCCL
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    from tests.test_facade_gpu import gen
    P = orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = next(gen(4, 32, 64, 4, onehot=False))
    e = Engine(20, widths=SMALL, device_id=rank, seed=7)
    if rank != 0:                                   # rank 0's parameters must arrive through the broadcast, not through the shared seed
        P = {k: np.zeros_like(v) for k, v in P.items()}
    e.set_params(P)
    if native:
        e.comm_init_native()
        assert e.comm_info()["world"] == world and e.comm_info()["rank"] == rank
    e.broadcast_params(0)
    sl = slice(2 * rank, 2 * rank + 2)
    loss, step = e.train_step(img[sl], lab[sl], 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
    e.metrics_reset(); e.eval_step(img[sl], lab[sl]); e.metrics_allreduce()
    out[rank] = (e.flat_params.cpu().numpy(), loss, step, int(e.metrics_raw()[0].sum()), e.metrics_raw()[2])
    if native:
        assert L.lib.fcn8s_comm_destroy(e.h) == 0
    e.close()
    dist.destroy_process_group()


@needs2
@pytest.mark.parametrize("native", [False, True], ids=["torch.distributed", "native fcn8s_comm"])
def test_two_rank_rccl_step_equals_big_batch_step(native):
    """tests/test_facade_gpu.py::test_two_rank_data_parallel_step_equals_big_batch_step over RCCL, one rank per GPU: the replicas end
    bit-identical, rank 1 received rank 0's parameters through the broadcast, the update equals the update of one process stepping on the
    whole batch, the confusion matrix and the loss samples are summed over the ranks."""
    import socket
    import torch.multiprocessing as mp
    from fcn8s_tensorflow_amd.engine import Engine
    from fcn8s_tensorflow_amd import _lib as L
    from tests.test_facade_gpu import gen
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_rccl_worker, args=(2, port, native, out), nprocs=2, join=True)
    p0, p1 = out[0][0], out[1][0]
    np.testing.assert_array_equal(p0, p1)
    assert out[0][2] == out[1][2] == 1
    assert out[0][3] == 4 * 32 * 64 and out[0][4] == 2
    P = orc.init_params(20, SMALL, seed=1, decoder_std_scale=30.0, bias_std=0.05)
    img, lab = next(gen(4, 32, 64, 4, onehot=False))
    e = Engine(20, widths=SMALL); e.set_params(P)
    before = e.flat_params.cpu().numpy().copy()
    e.train_step(img, lab, 1e-2, keep_prob=1.0, l2_rate=1e-3, optimizer=L.OPT_SGD_MOMENTUM)
    ref = e.flat_params.cpu().numpy()
    e.close()
    upd_ref, upd_dp = ref - before, p0 - before
    assert np.abs(upd_ref).max() > 0
    assert np.abs(upd_dp - upd_ref).max() <= 2e-3 * np.abs(upd_ref).max()


@needs2
def test_a_dead_rank_ends_the_run_with_an_error_line():
    """Rank 1 raises after its warm-up steps (FCN8S_BENCH_FAIL_RANK): rank 0 is then waiting in a collective for a peer that is gone.  The
    run must END (launcher SIGTERM -> rank 0's watcher thread, or the process-group timeout) and stdout must hold exactly one JSON line whose
    `error` says why."""
    env = _env(); env["FCN8S_BENCH_FAIL_RANK"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--repeats", "1", "--batch", "2",
                        "--height", "64", "--width", "64", "--no-cpu-baseline", "--rank-timeout", "60"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0
    out = _json_line(r.stdout)
    assert out["value"] is None and out["error"] and out["n_gpus"] == 2, out


def test_a_dead_rank_ends_the_run_with_an_error_line_on_one_gpu():
    """The same over gloo with both ranks on the one GPU (runs on every box)."""
    env = _env(); env["FCN8S_BENCH_FAIL_RANK"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--device", "0", "--steps", "3", "--warmup", "1",
                        "--repeats", "1", "--batch", "2", "--height", "64", "--width", "64", "--no-cpu-baseline", "--rank-timeout", "60"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0
    out = _json_line(r.stdout)
    assert out["value"] is None and out["error"] and out["n_gpus"] == 2, out


def test_the_multi_gpu_tests_say_why_they_were_skipped():
    """On a one-GPU box the N-rank tests above are skipped, not silently absent: this test prints the count that gates them."""
    n = _ngpus()
    print("torch.cuda.device_count() = %d: the N-rank RCCL tests of this file %s" % (n, "RUN" if n >= 2 else "are SKIPPED (need >= 2 GPUs)"))
    assert n >= 1
