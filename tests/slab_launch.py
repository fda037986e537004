"""How the multi-rank tests start their workers: one process per rank under torch.distributed.run on 127.0.0.1, all sharing the one
GPU of the test machine.  A worker (tests/*_worker.py) takes the mode as its argument and prints "WORKER_OK <rank>" on success."""
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_workers(worker, mode, nproc, timeout, extra_env=None, tail=6000):
    """`nproc` ranks of tests/<worker> in `mode`; every rank must report success.  Returns the ranks' output; on failure the last
    `tail` characters of it are the assertion's message."""
    cmd = [
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
        "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(HERE, worker), mode,
    ]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.update(extra_env or {})
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout, env=env)
    ok = [f"WORKER_OK {r}" in res.stdout for r in range(nproc)]
    assert res.returncode == 0 and all(ok), res.stdout[-tail:]
    return res.stdout
