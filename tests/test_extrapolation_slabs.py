"""Velocity extrapolation on Z-slabs (include/mgps_fields.h): 2 and 4 ranks share the one device over
TorchDistComm/gloo (tests/extrapolate_slab_worker.py, one process per rank) and must reproduce mgps_fields_extrapolate3 on their
planes bit for bit; one rank over RcclComm extrapolates behind the one-call projection; a transport whose exchange fails gives
MGPS_ERR_COMM.  Every launch has a timeout of its own."""
from functools import partial
import pytest

from slab_launch import run_workers as launch

run_workers = partial(launch, "extrapolate_slab_worker.py")


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


@pytest.mark.gpu
def test_missing_array_on_one_rank_is_refused_on_every_rank():
    print(run_workers("missing", 2, 120)[-2000:])
