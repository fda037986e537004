"""options.enclosed_liquid on slab solvers.  2 and 4 ranks share the one GPU over TorchDistComm/gloo (tests/enclosed_slab_worker.py,
one process per rank) and must reproduce the single-device solver on the whole grid: the component ranks entry for entry (sealed
tank, pockets sealed on and next to a cut, a serpentine across every cut, a far DIRICHLET contact, DIRICHLET across a cut behind
open and closed faces, 100+ bubbles, random domains, uneven cuts, the host builder), MG-PCG in every CG vector mode with both
smoothers and the diagonal preconditioner, the V-cycle and P.  Without pockets the option adds no bit, exchange or device
all-reduce.  A transport without gatherv / scatterv is refused."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

from slab_launch import run_workers as launch

run_workers = partial(launch, "enclosed_slab_worker.py")


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_ranks_match_whole_grid(nproc):
    print(run_workers("ranks", nproc, 300)[-2000:])


@pytest.mark.gpu
def test_slab_pcg_matches_single_device():
    print(run_workers("solve", 2, 300)[-2000:])


@pytest.mark.gpu
def test_slab_vcycle_and_projection():
    print(run_workers("cycle", 4, 240)[-1000:])


@pytest.mark.gpu
def test_slab_without_pockets_adds_nothing():
    print(run_workers("m0", 2, 300)[-1000:])


@pytest.mark.gpu
def test_slab_refused_without_gatherv():
    run_workers("refuse", 2, 120)


def test_slab_transport_too_short_for_the_merge_is_refused():
    """CPU: a transport whose struct_size ends before gatherv / scatterv cannot carry the merge of options.enclosed_liquid; the
    constructor refuses it before it touches a device"""
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import domains as D
    from geometricmultigridpressuresolver_amd._lib import lib
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    n = 32
    lab = np.full((n, n, n), D.EXTERIOR, dtype=np.uint8)
    lab[4:-4, 4:-4, 4:-4] = D.INTERIOR
    w = [np.ones(D.face_shape(n, n, n, a), dtype=np.float32) for a in range(3)]
    o = G.default_options()
    o.enclosed_liquid = 1
    comm = CommStruct()
    comm.struct_size = CommStruct.gatherv.offset  # (an older transport: everything up to destroy)
    comm.size = 1
    h = C.c_void_p()
    st = lib().mgps_create_slab(C.byref(h), n, n, n, lab.ctypes.data_as(C.c_void_p), *[a.ctypes.data_as(C.c_void_p) for a in w], 3, 0,
                                C.byref(o), C.byref(comm))
    assert st == 1 and not h.value
    msg = lib().mgps_last_error(None)
    assert b"options.enclosed_liquid" in msg and b"gatherv" in msg, msg
