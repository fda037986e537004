"""Velocity extrapolation on Z-slabs (include/mgps_fields.h): 2 and 4 ranks share the one device over
TorchDistComm/gloo (tests/extrapolate_slab_worker.py, one process per rank) and must reproduce mgps_fields_extrapolate3 on their
planes bit for bit; one rank over RcclComm extrapolates behind the one-call projection; a transport whose exchange fails gives
MGPS_ERR_COMM.  Every launch has a timeout of its own."""
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_workers(mode, nproc, timeout):
    cmd = [
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
        "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, "extrapolate_slab_worker.py"), mode,
    ]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env)
    ok = [f"WORKER_OK {r}" in res.stdout for r in range(nproc)]
    assert res.returncode == 0 and all(ok), res.stdout[-6000:]
    return res.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_extrapolation_is_bit_equal_to_single_device(nproc):
    print(run_workers("slabs", nproc, 300)[-3000:])


@pytest.mark.gpu
def test_one_rank_over_rccl_extrapolates_behind_the_projection():
    print(run_workers("one", 1, 300)[-2000:])


@pytest.mark.gpu
def test_failing_exchange_returns_comm_error_without_hanging():
    print(run_workers("fail", 2, 120)[-2000:])
