"""Slab solvers from the rank's own label planes on the device (mgps_create_slab_device_labels), the one-call slab projection built
on it and the cuts from label windows (mgps_slab_partition_device): the argument checks on the CPU; on the GPU the plane counts
against numpy, and 2 and 4 ranks sharing the one device over TorchDistComm/gloo plus one rank over RcclComm
(tests/slab_window_worker.py, one process per rank, several checks per launch)."""
import ctypes as C
from functools import partial

import numpy as np
import pytest

from slab_launch import run_workers as launch

run_workers = partial(launch, "slab_window_worker.py")


# ---- CPU: no device is touched --------------------------------------------------------------------------------------------------
N = 32


def _domain():
    from geometricmultigridpressuresolver_amd import domains as D

    lab = np.full((N, N, N), D.EXTERIOR, dtype=np.uint8)
    lab[4:-4, 4:-4, 4:-4] = D.INTERIOR
    return lab, [np.ones(D.face_shape(N, N, N, a), dtype=np.float32) for a in range(3)]


def _comm(size=1):
    """a complete vtable whose entries are never reached by a refused call"""
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    comm = CommStruct()
    comm.struct_size, comm.size = C.sizeof(CommStruct), size
    keep = [type(comm.exchange)(lambda *a: 1), type(comm.allreduce)(lambda *a: 1), type(comm.gather)(lambda *a: 1), type(comm.scatter)(lambda *a: 1)]
    comm.exchange, comm.allreduce, comm.gather, comm.scatter = keep
    return comm, keep


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _create(lab, w, opt, comm, cuts, labels=True):
    import geometricmultigridpressuresolver_amd as G

    h = C.c_void_p()
    st = G.lib().mgps_create_slab_device_labels(C.byref(h), N, N, N, _p(lab) if labels else None, _p(w[0]), _p(w[1]), _p(w[2]), 3, 0,
                                                C.byref(opt) if opt is not None else None, C.byref(comm) if comm is not None else None, cuts)
    assert not h.value
    return st, G.lib().mgps_last_error(None).decode()


def test_symbols_resolve():
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd.distributed import SlabSolver, slab_partition_device

    assert all(hasattr(G.lib(), name) for name in ("mgps_create_slab_device_labels", "mgps_slab_partition_device", "mgps_label_plane_counts"))
    assert callable(SlabSolver.from_device_labels) and callable(slab_partition_device)


def test_constructor_refuses_bad_arguments():
    """the labels are never read here (the pointers are host arrays): every refusal comes before any device work"""
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    lab, w = _domain()
    cuts = (C.c_int * 2)(0, N)
    comm, keep = _comm()
    st, msg = _create(lab, w, G.default_options(), comm, cuts, labels=False)
    assert st == 1 and "label planes are required" in msg, msg
    st, msg = _create(lab, w, G.default_options(), comm, None)
    assert st == 1 and "cuts are required" in msg, msg
    st, msg = _create(lab, w, G.default_options(), None, cuts)
    assert st == 1 and "comm" in msg, msg
    bare = CommStruct()
    bare.struct_size, bare.size = C.sizeof(CommStruct), 1  # (no entry set)
    st, msg = _create(lab, w, G.default_options(), bare, cuts)
    assert st == 1 and "incomplete mgps_comm" in msg, msg
    st, msg = _create(lab, w, G.default_options(), comm, (C.c_int * 2)(0, N - 2))
    assert st == 1 and "cuts must run from 0 to nz" in msg, msg
    o = G.default_options()
    o.precision = 1
    st, msg = _create(lab, w, o, comm, cuts)
    assert st == 1 and "precision" in msg, msg


def test_constructor_refuses_host_setup():
    """the host builder reads the whole grid: refused by name, by every rank alike (options are shared), before any collective"""
    import geometricmultigridpressuresolver_amd as G

    lab, w = _domain()
    o = G.default_options()
    o.host_setup = 1
    comm, keep = _comm()
    st, msg = _create(lab, w, o, comm, (C.c_int * 2)(0, N))
    assert st == 1 and "host_setup" in msg, msg


def test_constructor_transport_too_short_for_the_merge_is_refused():
    """options.enclosed_liquid with a transport whose struct_size ends before gatherv / scatterv, as
    tests/test_enclosed_slabs.py::test_slab_transport_too_short_for_the_merge_is_refused checks it on mgps_create_slab"""
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    lab, w = _domain()
    o = G.default_options()
    o.enclosed_liquid = 1
    comm = CommStruct()
    comm.struct_size, comm.size = CommStruct.gatherv.offset, 1
    st, msg = _create(lab, w, o, comm, (C.c_int * 2)(0, N))
    assert st == 1 and "options.enclosed_liquid" in msg and "gatherv" in msg, msg


def test_partition_refuses_bad_arguments():
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    lab, _ = _domain()
    comm, keep = _comm(2)
    now, out = (C.c_int * 3)(0, N // 2, N), (C.c_int * 3)()
    o = G.default_options()

    def call(labels, cuts, cm, dst):
        st = G.lib().mgps_slab_partition_device(N, N, N, labels, cuts, 3, 0, C.byref(o), C.byref(cm) if cm is not None else None, dst)
        return st, G.lib().mgps_last_error(None).decode()

    for args in ((None, now, comm, out), (_p(lab), None, comm, out), (_p(lab), now, None, out), (_p(lab), now, comm, None)):
        st, msg = call(*args)
        assert st == 1 and "are required" in msg, msg
    bare = CommStruct()
    bare.struct_size, bare.size = C.sizeof(CommStruct), 2
    st, msg = call(_p(lab), now, bare, out)
    assert st == 1 and "incomplete mgps_comm" in msg, msg
    st, msg = call(_p(lab), (C.c_int * 3)(0, N, N), comm, out)
    assert st == 1 and "cuts must run from 0 to nz" in msg, msg


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 36, 50), (5, 37, 51), (3, 250, 300), (2, 16, 16)])
def test_plane_counts_match_numpy(shape):
    """planes of 1800 and 1887 bytes (no multiple of 16: every plane starts at another alignment, odd ones included), of 75000
    (two workgroups per plane, 8 bytes behind the last 16-byte load) and of 256 (no head, no tail); a view that starts one byte
    into the allocation moves every alignment again"""
    import torch

    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd._lib import check

    nz, ny, nx = shape
    rng = np.random.default_rng(nx)
    for shift in (0, 1):
        lab = rng.integers(0, 4, size=shape, dtype=np.uint8)
        buf = torch.zeros(lab.size + shift, dtype=torch.uint8, device="cuda")
        buf[shift:] = torch.from_numpy(lab.ravel()).cuda()
        torch.cuda.synchronize()
        act, bnd = (C.c_int64 * nz)(), (C.c_int64 * nz)()
        check(G.lib().mgps_label_plane_counts(nx, ny, nz, C.c_void_p(buf.data_ptr() + shift), act, bnd))
        assert list(act) == [int(((p == 0) | (p == 3)).sum()) for p in lab], (shape, shift)
        assert list(bnd) == [int((p == 3).sum()) for p in lab], (shape, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_label_windows_on_ranks(nproc):
    print(run_workers("ranks", nproc, 420)[-5000:])


@pytest.mark.gpu
def test_label_windows_on_one_rank_over_rccl():
    print(run_workers("one", 1, 300)[-2000:])
