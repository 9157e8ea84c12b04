"""bench.py's N-rank launch (VERDICT r2 "missing 2"): `bench.py --gpus N`
without a launcher starts N ranks itself, and any failure -- a rank dying, a
WORLD_SIZE that disagrees with --gpus, too few GPUs for RCCL -- is a non-zero
exit with no result line, never a one-GPU line under an N-GPU label.

CPU tests run the launcher with --launch-probe (ranks rendezvous over gloo and
report, no GPU); the GPU test runs real N = 2 steps with both ranks on the
box's one device (NMP_BENCH_BACKEND=gloo, the rehearsal backend)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, timeout=180, **env):
    e = dict(os.environ, **env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        if k not in env:
            e.pop(k, None)
    p = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True,
                       timeout=timeout, env=e)
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    return p.returncode, lines, p.stderr


@pytest.mark.parametrize("n", [2, 3, 8])
def test_spawned_ranks_report_world(n):
    rc, lines, err = run(["--gpus", str(n), "--launch-probe", "--ncol", "500"])
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    ln = lines[0]
    assert ln["n_gpus"] == n and ln["ranks_joined"] == n
    assert ln["ncol_total"] == n * 500 and ln["first_col_sum"] == 500 * n * (n - 1) // 2


def test_torchrun_eight_ranks_report_world():
    """The driver's own N = 8 launch line (torch.distributed.run, one process
    per rank, rendezvous on 127.0.0.1) with --launch-probe: eight ranks join,
    rank 0 alone prints one line with n_gpus 8 and every rank's block."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    e = {k: v for k, v in os.environ.items()
         if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port",
                        str(port), BENCH, "--gpus", "8", "--launch-probe", "--ncol", "300"],
                       capture_output=True, text=True, timeout=300, env=e)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, lines
    ln = lines[0]
    assert ln["n_gpus"] == 8 and ln["ranks_joined"] == 8
    assert ln["ncol_total"] == 8 * 300 and ln["first_col_sum"] == 300 * 8 * 7 // 2


def test_failed_rank_fails_the_job():
    rc, lines, err = run(["--gpus", "2", "--launch-probe", "--ncol", "500"],
                         NMP_BENCH_FAIL_RANK="1")
    assert rc != 0 and not lines
    assert "rank 1 exited" in err


def test_world_size_must_match_gpus():
    rc, lines, err = run(["--gpus", "4", "--launch-probe", "--ncol", "500"], WORLD_SIZE="1",
                         RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29555")
    assert rc != 0 and not lines and "WORLD_SIZE 1" in err


def test_rccl_needs_one_gpu_per_rank():
    """With the default backend (RCCL) the launcher counts devices first: this
    container has none, so --gpus 2 must fail before starting any rank."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("enough GPUs here")
    rc, lines, err = run(["--gpus", "2", "--ncol", "500", "--no-cpu-baseline"])
    assert rc == 2 and not lines and "visible GPUs" in err


@pytest.mark.gpu
def test_bench_two_ranks_on_the_gpu():
    """A real N = 2 bench line from `bench.py --gpus 2` alone: both ranks step
    their shard through the HIP engine (sharing the box's one GPU; gloo for the
    gather), output every step gathered to rank 0."""
    rc, lines, err = run(["--gpus", "2", "--ncol", "8192", "--steps", "4", "--warmup", "1",
                          "--out-every", "2", "--no-cpu-baseline", "--period", "4"],
                         timeout=240, NMP_BENCH_BACKEND="gloo")
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    ln = lines[0]
    assert ln["n_gpus"] == 2 and ln["config"]["ncol_total"] == 2 * 8192
    assert ln["value"] > 0 and ln["checks"]["stc_finite"]
    assert ln["config"]["backend"] == "gloo"


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run times exactly --steps steps, leaves the
    CPU baseline to --full, and with --dump-outputs writes what the last timed
    step left (state, ISNOW, status, the last output step's 16 diagnostics) as
    float32 .npy files of the run's columns."""
    import numpy as np
    n = 8192
    rc, lines, err = run(["--gpus", "1", "--ncol", str(n), "--steps", "3", "--warmup", "1",
                          "--out-every", "2", "--period", "4", "--dump-outputs", str(tmp_path)],
                         timeout=240)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    ln = lines[0]
    assert ln["steps"] == 3 and ln["warmup"] == 1 and ln["cpu_baseline"] is None
    assert ln["ms_per_step"] > 0 and ln["dtype"] == "f32"
    assert abs(ln["value"] * ln["ms_per_step"] * 1e-3 - n) < 1e-6 * n
    got = {p.name: np.load(p) for p in tmp_path.glob("*.npy")}
    shapes = {"state.npy": (56, n), "diag.npy": (16, n), "isnow.npy": (n,), "status.npy": (n,),
              "columns.npy": (n,)}
    assert {k: v.shape for k, v in got.items()} == shapes
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["state.npy"].dtype == np.float32 and np.isfinite(got["diag.npy"]).all()
    assert (got["columns.npy"] == np.arange(n)).all() and (got["status.npy"] == 0).all()
    assert set(np.unique(got["isnow.npy"])) <= {0.0, -1.0, -2.0, -3.0}


@pytest.mark.parametrize("how", ["SIGTERM", "SIGKILL"])
def test_launcher_death_takes_the_ranks_down(tmp_path, how):
    """The ranks run in their own sessions; if the launcher is stopped (a
    signal, a driver's timeout) or killed outright, no rank may outlive it
    holding the GPU: SIGTERM is forwarded to every rank's process group, and
    each rank has PR_SET_PDEATHSIG for the launcher's SIGKILL."""
    import signal
    import time
    e = dict(os.environ, NMP_BENCH_HANG_DIR=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.Popen([sys.executable, BENCH, "--gpus", "2", "--launch-probe", "--ncol", "100"],
                         env=e, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    pids = []
    for _ in range(600):
        files = sorted(tmp_path.glob("rank*.pid"))
        if len(files) == 2 and all(f.read_text() for f in files):
            pids = [int(f.read_text()) for f in files]
            break
        time.sleep(0.1)
    try:
        assert len(pids) == 2, "ranks did not start"
        p.send_signal(getattr(signal, how))
        p.wait(timeout=30)

        def alive(pid):
            try:
                os.kill(pid, 0)
            except ProcessLookupError:
                return False
            # a zombie awaiting its reaper is gone for our purposes
            try:
                with open(f"/proc/{pid}/stat") as f:
                    return f.read().split(")")[-1].split()[0] != "Z"
            except FileNotFoundError:
                return False
        for _ in range(100):
            if not any(alive(q) for q in pids):
                break
            time.sleep(0.1)
        assert not any(alive(q) for q in pids), "a rank outlived the launcher"
    finally:
        for q in pids:
            try:
                os.kill(q, signal.SIGKILL)
            except ProcessLookupError:
                pass
