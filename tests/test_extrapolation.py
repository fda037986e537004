"""Velocity extrapolation into the air band (include/mgps_fields.h): the numpy restatement
(tests/extrapolation_reference.py) against an independent breadth-first search on the CPU, the argument refusals of the C ABI without
a device, and on the GPU mgps_fields_extrapolate / mgps_fields_extrapolate3 against the restatement.

Tolerance (derived, extrapolation_reference.bound): a layer costs at most 5 additions and one division and a mean does not expand the
max norm, so |device - float64 restatement| <= 8 * L * 2^-24 * max|v| after L layers.  Layer grids, untouched faces and the filled
counts are compared exactly; equality of the values with the float32 restatement is printed, not asserted."""
import ctypes as C

import numpy as np
import pytest

import extrapolation_reference as R
from refusals import refused as _refused

SHAPE = (24, 20, 28)  # (gz, gy, gx)
L = 6


def face_shape(shape, axis):
    s = list(shape)
    s[2 - axis] += 1
    return tuple(s)


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cw", [True, False])
def test_restatement_layer_is_breadth_first_distance(with_cw):
    sc, valid = R.scene(SHAPE)
    ref = R.scene_reference(SHAPE, L, with_cw, False)
    for a in range(3):
        cw = sc["cut_weights"][a] if with_cw else None
        assert np.array_equal(ref[a][1], R.bfs_distance(valid[a], L, cw)), a
        # the non-vacuity condition of the GPU tests: every layer fills a shell worth the name
        assert min(ref[a][2]) >= 500, (a, ref[a][2])
        assert [int((ref[a][1] == l).sum()) for l in range(1, L + 1)] == ref[a][2]
        untouched = (ref[a][1] == 0) | (ref[a][1] == R.OPEN)
        assert np.array_equal(ref[a][0][untouched], sc["velocity"][a][untouched])
        if with_cw:
            assert not (ref[a][1][~(cw > 0)] % R.OPEN).any()  # closed faces: valid never, reached never


@pytest.mark.parametrize("with_cw", [True, False])
def test_restatement_carries_a_constant_exactly(with_cw):
    sc, valid = R.scene(SHAPE)
    rng = np.random.default_rng(5)
    for a in range(3):
        v = np.where(valid[a] == 1, np.float32(-2.0), rng.random(valid[a].shape, dtype=np.float32) + 1)
        out, layer, _ = R.extrapolate(v, valid[a], L, sc["cut_weights"][a] if with_cw else None)
        reached = (layer > 0) & (layer < R.OPEN)
        assert reached.sum() > 3000 and (out[reached] == np.float32(-2.0)).all()
        assert np.array_equal(out[~reached], v[~reached])


def test_restatement_float32_against_float64():
    sc, _ = R.scene(SHAPE)
    for with_cw in (True, False):
        r32, r64 = R.scene_reference(SHAPE, L, with_cw, False), R.scene_reference(SHAPE, L, with_cw, True)
        for a in range(3):
            assert np.array_equal(r32[a][1], r64[a][1]) and r32[a][2] == r64[a][2]
            err, lim = np.abs(r32[a][0] - r64[a][0]).max(), R.bound(L, np.abs(sc["velocity"][a]).max())
            print(f"float32 against float64 restatement, cut weights {with_cw}, axis {a}: {err:.2e} (bound {lim:.2e})")
            assert err <= lim


# ---- CPU: the C ABI refuses bad arguments on the host, before any HIP call -------------------------------------------------------------
def test_argument_refusals_need_no_device():
    from geometricmultigridpressuresolver_amd._lib import lib

    p = C.c_void_p(64)  # (never dereferenced: every call below is refused on the host)
    p3 = (C.c_void_p * 3)(64, 64, 64)
    two = (C.c_void_p * 3)(64, None, 64)
    one = lib().mgps_fields_extrapolate
    for layers in (0, 255, -3):
        _refused(one(0, p, p, p, None, layers, 4, 4, 4, None), "mgps_fields_extrapolate", "layers", "1 .. 254")
    for axis in (-1, 3):
        _refused(one(axis, p, p, p, None, 2, 4, 4, 4, None), "axis", "0 .. 2")
    for g in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        _refused(one(0, p, p, p, None, 2, *g, None), "extent")
    _refused(one(0, None, p, p, None, 2, 4, 4, 4, None), "velocity")
    _refused(one(0, p, None, p, None, 2, 4, 4, 4, None), "layer")
    _refused(one(0, p, p, None, None, 2, 4, 4, 4, None), "valid")
    three = lib().mgps_fields_extrapolate3
    _refused(three(p3, p3, p3, None, 255, 4, 4, 4, None, None), "mgps_fields_extrapolate3", "layers")
    _refused(three(p3, p3, p3, None, 2, 4, 0, 4, None, None), "extent")
    _refused(three(two, p3, p3, None, 2, 4, 4, 4, None, None), "velocity")
    _refused(three(None, p3, p3, None, 2, 4, 4, 4, None, None), "velocity")
    _refused(three(p3, two, p3, None, 2, 4, 4, 4, None, None), "layer")
    _refused(three(p3, p3, two, None, 2, 4, 4, 4, None, None), "valid")
    _refused(three(p3, p3, p3, two, 2, 4, 4, 4, None, None), "cut_weights")


def _comm_of_one():
    from geometricmultigridpressuresolver_amd.distributed import CommStruct

    comm = CommStruct()
    comm.struct_size, comm.size = C.sizeof(CommStruct), 1
    keep = [type(comm.exchange)(lambda *a: 1), type(comm.allreduce)(lambda *a: 1)]  # (a complete vtable; never called: a world of one)
    comm.exchange, comm.allreduce = keep
    return comm, keep


def test_slab_entries_refuse_on_the_host_and_the_mirror_has_the_library_size():
    from geometricmultigridpressuresolver_amd import fields as F
    from geometricmultigridpressuresolver_amd._lib import lib

    call = lib().mgps_extrapolate_velocity_slab
    comm, keep = _comm_of_one()
    cuts = (C.c_int * 2)(0, 128)
    ex = F.ExtrapolationSlab()
    ex.struct_size = C.sizeof(F.ExtrapolationSlab)
    ex.gx, ex.gy, ex.gz, ex.power_of_two, ex.layers = 64, 64, 96, 1, 0
    # the mirror's size is the library's: the call gets as far as the next check; a mirror of another size is refused as such
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "mgps_extrapolate_velocity_slab", "layers")
    ex.struct_size -= 8
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "struct_size")
    ex.struct_size += 8
    ex.layers = 255
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "layers")
    ex.layers, ex.gy = 3, 0
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "extent")
    ex.gy = 64
    _refused(call(C.byref(ex), None, cuts, None), "comm")
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "velocity")  # (all NULL)
    for a in range(3):
        ex.velocity[a] = 64
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "valid_faces")
    for a in range(3):
        ex.valid_faces[a] = 64
    ex.cut_weights[1] = 64
    _refused(call(C.byref(ex), C.byref(comm), cuts, None), "cut_weights")
    # the slab pass
    d = F.slab_window((96, 64, 64), True, [0, 64, 128], 0)
    p3 = (C.c_void_p * 3)(64, 64, 64)
    two = (C.c_void_p * 3)(64, 64, None)
    layer = lib().mgps_fields_slab_extrapolate_layer
    _refused(layer(C.byref(d), 255, p3, p3, p3, None, None, None, None, None, None, None), "mgps_fields_slab_extrapolate_layer", "l = 255")
    _refused(layer(C.byref(d), 1, two, p3, None, None, p3, None, p3, None, None, None), "velocity")
    _refused(layer(C.byref(d), 1, p3, None, None, None, p3, None, p3, None, None, None), "layer")
    _refused(layer(C.byref(d), 0, p3, p3, None, None, None, None, None, None, None, None), "valid")
    _refused(layer(C.byref(d), 1, p3, p3, None, None, None, None, None, None, None, None), "velocity_hi")  # (rank 0 of 2: a rank above)
    _refused(layer(C.byref(d), 1, p3, p3, None, None, p3, None, p3, two, None, None), "cut_weights")
    d.struct_size -= 4
    _refused(layer(C.byref(d), 1, p3, p3, None, None, p3, None, p3, None, None, None), "struct_size")


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _single_axis(axis, velocity, valid, cw, layers, shape, misalign=(0, 0)):
    """mgps_fields_extrapolate through lib() on copies; layer and valid start `misalign` bytes into their buffers"""
    import torch

    from geometricmultigridpressuresolver_amd._lib import check, lib

    n = velocity.size
    v = _dev(velocity)
    lay_buf, val_buf = torch.empty(n + 8, dtype=torch.uint8, device="cuda"), torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    lay, val = lay_buf[misalign[0]:misalign[0] + n], val_buf[misalign[1]:misalign[1] + n]
    val.copy_(_dev(valid).reshape(-1))
    w = _dev(cw) if cw is not None else None
    gz, gy, gx = shape
    check(lib().mgps_fields_extrapolate(axis, C.c_void_p(v.data_ptr()), C.c_void_p(lay.data_ptr()), C.c_void_p(val.data_ptr()),
                                        C.c_void_p(w.data_ptr()) if w is not None else None, int(layers), gx, gy, gz, None))
    torch.cuda.synchronize()
    return v.cpu().numpy(), lay.cpu().numpy().reshape(velocity.shape)


def _check_against_restatement(what, got_v, got_layer, velocity, ref32, ref64, layers):
    """layer exactly, untouched faces bit for bit, values within the derived bound of the float64 restatement"""
    assert np.array_equal(got_layer, ref64[1]), what
    untouched = (ref64[1] == 0) | (ref64[1] == R.OPEN)
    assert np.array_equal(got_v[untouched].view(np.uint32), velocity[untouched].view(np.uint32)), what
    err, lim = float(np.abs(got_v - ref64[0]).max()), R.bound(layers, float(np.abs(velocity).max()))
    print(f"{what}: max error {err:.2e} (bound {lim:.2e}), equal to the float32 restatement: {np.array_equal(got_v, ref32[0])}")
    assert err <= lim, (what, err, lim)


@pytest.mark.gpu
@pytest.mark.parametrize("with_cw", [True, False])
@pytest.mark.parametrize("layers", [1, 3, 6])
def test_whole_grid_matches_restatement(layers, with_cw):
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    sc, valid = R.scene(SHAPE)
    ref32, ref64 = R.scene_reference(SHAPE, layers, with_cw, False), R.scene_reference(SHAPE, layers, with_cw, True)
    cw = sc["cut_weights"] if with_cw else None
    vel = [_dev(a) for a in sc["velocity"]]
    layer, filled = F.extrapolateVelocity(vel, [_dev(a) for a in valid], layers, [_dev(a) for a in cw] if with_cw else None)
    torch.cuda.synchronize()
    for a in range(3):
        what = f"extrapolate3 L={layers} cut weights {with_cw} axis {a}"
        assert min(ref64[a][2]) >= 500, (what, ref64[a][2])  # non-vacuity: every layer fills a shell
        got_v, got_layer = vel[a].cpu().numpy(), layer[a].cpu().numpy()
        _check_against_restatement(what, got_v, got_layer, sc["velocity"][a], ref32[a], ref64[a], layers)
        assert filled[a] == sum(ref64[a][2]), (what, filled[a], ref64[a][2])
        one_v, one_layer = _single_axis(a, sc["velocity"][a], valid[a], cw[a] if with_cw else None, layers, SHAPE)
        _check_against_restatement(what.replace("extrapolate3", "extrapolate"), one_v, one_layer, sc["velocity"][a], ref32[a], ref64[a], layers)
        assert np.array_equal(one_v.view(np.uint32), got_v.view(np.uint32)) and np.array_equal(one_layer, got_layer), what


@pytest.mark.gpu
@pytest.mark.parametrize("with_cw", [True, False])
def test_ragged_small_grid(with_cw):
    """(9, 7, 13): rows of 13 and 14 faces, every grid edge, isolated sources; the single-axis entry also with layer and valid grids
    that do not start on a dword"""
    import torch

    from geometricmultigridpressuresolver_amd import fields as F

    shape, layers = (9, 7, 13), 4
    rng = np.random.default_rng(20)
    faces = [face_shape(shape, a) for a in range(3)]
    valid = [(rng.random(fs) < 0.05).astype(np.uint8) for fs in faces]
    velocity = [(rng.random(fs, dtype=np.float32) * 4 - 2) for fs in faces]
    cw = [(rng.random(fs) < 0.7).astype(np.float32) for fs in faces] if with_cw else None
    assert all(8 <= v.sum() < v.size // 10 for v in valid)
    vel = [_dev(a) for a in velocity]
    layer, filled = F.extrapolateVelocity(vel, [_dev(a) for a in valid], layers, [_dev(a) for a in cw] if with_cw else None)
    torch.cuda.synchronize()
    for a in range(3):
        c = cw[a] if with_cw else None
        ref32, ref64 = R.extrapolate(velocity[a], valid[a], layers, c), R.extrapolate(velocity[a], valid[a], layers, c, np.float64)
        assert np.array_equal(ref64[1], R.bfs_distance(valid[a], layers, c))
        edges = [ref64[1][sl] for sl in ((0,), (-1,), (slice(None), 0), (slice(None), -1), (Ellipsis, 0), (Ellipsis, -1))]
        assert all(((e > 0) & (e < R.OPEN)).any() for e in edges), "a grid edge without a filled face"
        what = f"ragged cut weights {with_cw} axis {a}"
        _check_against_restatement(what, vel[a].cpu().numpy(), layer[a].cpu().numpy(), velocity[a], ref32, ref64, layers)
        assert filled[a] == sum(ref64[2]), (what, filled[a], ref64[2])
        for mis in ((1, 3), (2, 2), (3, 0)):
            one_v, one_layer = _single_axis(a, velocity[a], valid[a], c, layers, shape, mis)
            assert np.array_equal(one_v.view(np.uint32), vel[a].cpu().numpy().view(np.uint32)) and np.array_equal(one_layer, layer[a].cpu().numpy()), (what, mis)


@pytest.mark.gpu
def test_uint8_layer_cap():
    """(1, 1, 300), x-faces, one source at face 0, L = 254: faces 1 .. 254 carry layers 1 .. 254 and the source's value; faces
    255 .. 300 stay as they were with layer 255.  L = 255 is refused."""
    from geometricmultigridpressuresolver_amd import MgpsError

    shape, layers = (1, 1, 300), 254
    rng = np.random.default_rng(3)
    velocity = rng.random((1, 1, 301), dtype=np.float32) + 1
    velocity[0, 0, 0] = np.float32(0.7)
    valid = np.zeros((1, 1, 301), dtype=np.uint8)
    valid[0, 0, 0] = 1
    got_v, got_layer = _single_axis(0, velocity, valid, None, layers, shape)
    assert np.array_equal(got_layer[0, 0], np.concatenate([np.arange(255), np.full(46, 255)]).astype(np.uint8))
    err, lim = float(np.abs(got_v[0, 0, 1:255].astype(np.float64) - np.float64(np.float32(0.7))).max()), R.bound(layers, float(velocity.max()))
    print(f"uint8 cap: max error {err:.2e} (bound {lim:.2e}), exact: {err == 0.0}")
    assert err <= lim
    assert np.array_equal(got_v[0, 0, 255:].view(np.uint32), velocity[0, 0, 255:].view(np.uint32)) and got_v[0, 0, 0] == np.float32(0.7)
    with pytest.raises(MgpsError) as e:
        _single_axis(0, velocity, valid, None, 255, shape)
    assert e.value.status == 1 and "layers" in str(e.value)
