"""The fields layer on Z-slabs (include/mgps_fields.h): mgps_projection_slab_layout on the CPU; on the GPU
2 and 4 ranks share the one device over TorchDistComm/gloo (tests/projection_slab_worker.py, one process per rank) and must
reproduce the single-device passes on their planes and the single-device one-call projection of the same scene; one rank over
RcclComm is the device-resident projection.  Several checks run per worker launch to keep the suite short."""
import ctypes as C
from functools import partial

import pytest

from slab_launch import run_workers as launch

run_workers = partial(launch, "projection_slab_worker.py")


# grids whose ranks get at least 16 base planes each at 4 ranks: the 16-plane minimum of a rank then does not bind and the division of
# the base planes is left to the cut granule alone (the case where it binds: test_layout_where_the_plane_minimum_binds)
LAYOUT_SHAPES = [(96, 64, 64), (64, 64, 64), (200, 100, 100), (128, 40, 56), (480, 480, 480)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_layout_cuts(shape):
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    gz = shape[0]
    for p2 in (False, True):
        eshape, offset, levels = G.expanded_layout(shape, 0, power_of_two=p2)
        for size in (1, 2, 4):
            for gs in (False, True):
                lay = F.projection_slab_layout(shape, p2, size, gs)
                what = (shape, p2, size, gs, lay)
                assert lay["expanded"] == tuple(eshape) and lay["offset"] == offset and lay["levels"] == levels, what
                cuts, unit = lay["splits"], 16 if gs else 2
                assert len(cuts) == size + 1 and cuts[0] == 0 and cuts[-1] == eshape[0], what
                assert all(b > a for a, b in zip(cuts, cuts[1:])) and all(c % unit == 0 for c in cuts), what
                assert all(b - a >= 16 for a, b in zip(cuts, cuts[1:])), what
                base = [min(max(c - offset, 0), gz) for c in cuts]
                planes = [b - a for a, b in zip(base, base[1:])]
                assert min(planes) >= 1 and sum(planes) == gz and max(planes) - min(planes) <= unit, (what, planes)
                for r in range(size):  # the window every rank derives from them
                    d = F.slab_window(shape, p2, cuts, r)
                    assert (d.c0, d.c1, d.e0, d.e1) == (base[r], base[r + 1], cuts[r], cuts[r + 1]) and d.c0 < d.c1, what


def test_layout_where_the_plane_minimum_binds():
    """48 base planes behind an offset of 16, 4 ranks, Jacobi: an even division would be 12 base planes each, but an interior rank owns
    expanded planes that are all base planes and needs 16 of them.  The helper returns the most even cuts the minimum allows: the
    interior ranks at the minimum, the rest shared by the end ranks, whose windows reach into the padding"""
    from geometricmultigridpressuresolver_amd import fields as F

    for p2 in (False, True):
        lay = F.projection_slab_layout((48, 48, 48), p2, 4, False)
        cuts, offset = lay["splits"], lay["offset"]
        assert offset == 16 and cuts[:4] == [0, 24, 40, 56] and cuts[4] == lay["expanded"][0], lay
        base = [min(max(c - offset, 0), 48) for c in cuts]
        planes = [b - a for a, b in zip(base, base[1:])]
        assert planes == [8, 16, 16, 8] and all(b - a >= 16 and a % 2 == 0 for a, b in zip(cuts, cuts[1:])), (lay, planes)


def test_layout_refuses_a_grid_too_thin_for_the_ranks():
    import geometricmultigridpressuresolver_amd as G
    from geometricmultigridpressuresolver_amd import fields as F

    for shape, size, gs in (((40, 32, 48), 4, False), ((48, 48, 48), 4, True), ((32, 32, 32), 8, False)):
        with pytest.raises(G.MgpsError) as e:
            F.projection_slab_layout(shape, True, size, gs)
        assert e.value.status == 1 and f"cannot be cut for {size} ranks" in str(e.value), str(e.value)
    # the even cut of the expanded grid leaves the end ranks with padding only: such cuts are refused, by every rank alike
    for rank in range(4):
        with pytest.raises(G.MgpsError) as e:
            F.slab_window((48, 48, 48), True, [0, 32, 64, 96, 128], rank)
        assert e.value.status == 1 and "owns no plane of the base grid" in str(e.value)


def test_struct_sizes_are_unchanged_and_mirrored():
    """the slab entry points add structs of their own; mgps_options, mgps_projection and mgps_comm keep their sizes (Python mirrors
    and tests build them), and the Python mirrors of the new structs match the header's layout as the compiler sees it"""
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import Options, lib
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    assert (C.sizeof(Options), C.sizeof(F.Projection), C.sizeof(CommStruct)) == (96, 368, 96)
    # the library checks struct_size against its own sizeof: a mirror of another size is refused with that message
    d = F.FieldsSlab()
    cuts = (C.c_int * 2)(0, 128)
    assert lib().mgps_fields_slab_describe(C.byref(d), 64, 64, 96, 1, cuts, 1, 0) == 0 and d.struct_size == C.sizeof(F.FieldsSlab)
    pr = F.ProjectionSlab()
    pr.struct_size = C.sizeof(F.ProjectionSlab)
    pr.gx = pr.gy = pr.gz = 0  # (bad extents: refused by the layout, after the struct_size and transport tests)
    comm = CommStruct()
    comm.struct_size, comm.size = C.sizeof(CommStruct), 1
    keep = [type(comm.exchange)(lambda *a: 1), type(comm.allreduce)(lambda *a: 1)]  # (a complete vtable; never called here)
    comm.exchange, comm.allreduce = keep
    assert lib().mgps_project_free_surface_slab(C.byref(pr), None, C.byref(comm), cuts, None) == 1
    assert b"mgps_expanded_layout" in lib().mgps_last_error(None), lib().mgps_last_error(None)
    pr.struct_size -= 8
    assert lib().mgps_project_free_surface_slab(C.byref(pr), None, C.byref(comm), cuts, None) == 1
    assert b"struct_size" in lib().mgps_last_error(None)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_passes_match_whole_grid_passes(nproc):
    print(run_workers("passes", nproc, 300)[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [2, 4])
def test_slab_projection_matches_single_device(nproc):
    print(run_workers("onecall", nproc, 420)[-4000:])


@pytest.mark.gpu
def test_slab_projection_options():
    print(run_workers("options", 2, 300)[-2000:])


@pytest.mark.gpu
def test_slab_projection_edges():
    print(run_workers("edges", 2, 300)[-2000:])


@pytest.mark.gpu
def test_missing_array_on_one_rank_is_refused_on_every_rank():
    print(run_workers("missing", 2, 120)[-2000:])


@pytest.mark.gpu
def test_one_rank_over_rccl_is_the_device_resident_projection():
    print(run_workers("one", 1, 300)[-2000:])
