"""Pressure forces on Z-slabs (include/mgps_fields.h): 2 and 4 ranks share the one device over
TorchDistComm/gloo (tests/solid_forces_slab_worker.py, one process per rank) and every rank must hold the rows of the single-device
pass on the gathered fields -- within the reordering bound of an fp64 sum, the count exactly, the same bits on all ranks; one rank
over RcclComm behind the one-call projection equals the whole-grid pass bit for bit and makes no transport call; a transport whose
exchange fails gives MGPS_ERR_COMM; a rank that comes without one of its arrays makes every rank return the same refusal.  Every launch has a timeout of its own."""
from functools import partial
import pytest

from slab_launch import run_workers as launch

run_workers = partial(launch, "solid_forces_slab_worker.py")


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_forces_match_single_device(nproc):
    print(run_workers("slabs", nproc, 300)[-3000:])


@pytest.mark.gpu
def test_one_rank_over_rccl_behind_the_projection_is_bit_equal():
    print(run_workers("one", 1, 300)[-2000:])


@pytest.mark.gpu
def test_failing_exchange_returns_comm_error_without_hanging():
    print(run_workers("fail", 2, 120)[-2000:])


@pytest.mark.gpu
def test_missing_array_on_one_rank_is_refused_on_every_rank():
    print(run_workers("missing", 2, 120)[-2000:])
