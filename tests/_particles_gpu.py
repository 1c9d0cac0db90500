"""What the GPU tests of the particle operators share (tests/test_gpu_particles2d.py, _stress, _subgrid, _inject and tests/test_gpu_particles3d.py): the grid
they all use, the seeded clouds, the way a cloud gets to the device and back, and the bit-for-bit comparison.  Written once and generic in the number of axes:
a shape ni of two entries means the 2D operators and tests/_particles2d.py, of three the 3D ones and tests/_particles3d.py.  A plain module like _blocks.py;
the names keep their leading underscore so that the test files read as they did when each carried its own copy."""
import ctypes as C
import functools

import numpy as np
import pytest

import _particles2d as PT2
import _particles3d as PT3

D = (0.125, 0.09375, 0.0625)          # the spacings; a 2D test uses the first two entries of D and ORIGIN
ORIGIN = (0.25, -0.5, 1.0)
NXCELL = {2: 4, 3: 8}                 # seeded per cell, by the number of axes
MAX_XCELL = 12
SENTINEL = -7.0e30


def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    """a float64 array on the device, through a copy that keeps its layout: the cached cases are shared read-only, and torch does not take a read-only array"""
    from justrelax_jl_amd.arrays import from_numpy
    return from_numpy(np.array(a, dtype=np.float64, order="K"), _dev())


def _up_int(a):
    """the mask, column-major as the particle arrays are"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.T)).permute(*reversed(range(a.ndim))).to(_dev())


def _host_int(t):
    return np.ascontiguousarray(t.permute(*reversed(range(t.dim()))).contiguous().cpu().numpy().T)


def _handle():
    from justrelax_jl_amd import _lib
    return _lib.Handle(_dev().index)


@pytest.fixture(scope="module")
def h(jr):
    """a handle of the test module's own; a file that changes a tuning key has its own fixture, which puts the key back"""
    return _handle()


def _launches(h):
    return h.get_option("stat_particles_launches")


def _P(t):
    return C.c_void_p(t.data_ptr())


def _vec(ts):
    return (C.c_void_p * len(ts))(*(t.data_ptr() for t in ts))


# ---------------------------------------------------------------------------------------------- comparison
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _ndiff(got, want):
    return int((_bits(got) != _bits(want)).sum())


# ---------------------------------------------------------------------------------------------- grid, velocities, clouds
def _xvi(ni):
    """the vertex coordinates along every axis"""
    return tuple(ORIGIN[d] + np.arange(ni[d] + 1) * D[d] for d in range(len(ni)))


def _xi_vel(ni):
    """the node coordinates of every velocity component: vertices along its own axis, ghosted centres along the others"""
    nd = len(ni)
    gh = [ORIGIN[d] + (np.arange(ni[d] + 2) - 0.5) * D[d] for d in range(nd)]
    return tuple(tuple(_xvi(ni)[d] if d == c else gh[d] for d in range(nd)) for c in range(nd))


def _V(ni, *fs):
    """the velocity components from functions of the node coordinates, ghost layers included"""
    out = []
    for grids, f in zip(_xi_vel(ni), fs):
        X = np.meshgrid(*grids, indexing="ij")
        out.append(np.asfortranarray(f(*X) + 0.0 * X[0]))
    return tuple(out)


def _rotation(ni, courant=0.5):
    """a rigid rotation about the box centre (3D: about a tilted axis through it); dt = 1 and the fastest corner moves `courant` of the smallest spacing"""
    nd = len(ni)
    c = [ORIGIN[d] + 0.5 * ni[d] * D[d] for d in range(nd)]
    if nd == 2:
        w = courant * min(D[:2]) / np.hypot(0.5 * ni[0] * D[0], 0.5 * ni[1] * D[1])
        return _V(ni, lambda X, Y: -w * (Y - c[1]), lambda X, Y: w * (X - c[0]))
    half = np.array([0.5 * ni[d] * D[d] for d in range(3)])
    w = courant * min(D) / np.linalg.norm(half) * (np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    return _V(ni, lambda X, Y, Z: w[1] * (Z - c[2]) - w[2] * (Y - c[1]), lambda X, Y, Z: w[2] * (X - c[0]) - w[0] * (Z - c[2]),
              lambda X, Y, Z: w[0] * (Y - c[1]) - w[1] * (X - c[0]))


def _seeded(ni, seed, nxcell=None, max_xcell=MAX_XCELL, min_xcell=2):
    """the restatement's jittered cloud on the tests' grid"""
    nd = len(ni)
    rng = None if seed is None else np.random.default_rng(seed)
    nxcell = NXCELL[nd] if nxcell is None else nxcell
    if nd == 2:
        return PT2.init_particles(nxcell, max_xcell, min_xcell, _xvi(ni), ni, rng=rng)
    return PT3.init_particles(nxcell, max_xcell, min_xcell, *_xi_vel(ni), rng=rng)


@functools.lru_cache(maxsize=None)
def _cloud0(ni):
    """the seeded cloud and three particle fields: phases 1 .. 3 in slabs along x with a random sprinkle, a temperature, an identity.  Shared: take _cloud"""
    q = _seeded(ni, {2: 20261020, 3: 20261021}[len(ni)] + ni[0])
    rng = np.random.default_rng(7 + ni[0])
    a = q.active != 0
    ph = np.where(a, 1.0 + np.floor(3.0 * (q.px - q.x0) / (ni[0] * D[0])), 0.0)
    ph = np.where(a & (rng.random(a.shape) < 0.2), rng.integers(1, 4, a.shape).astype(np.float64), ph)
    pT = np.where(a, rng.uniform(300.0, 1600.0, a.shape), 0.0)
    pid = np.where(a, np.arange(a.size).reshape(a.shape) + 1.0, 0.0)
    return q, (ph, pT, pid)


def _cloud(ni):
    q, f = _cloud0(ni)
    return (PT2 if len(ni) == 2 else PT3).copy(q), tuple(x.copy() for x in f)


def _rotated(ni):
    """2D: another seeded cloud after one advect_rk2 + move under the rotation, shown lossless: buckets unevenly filled, inactive slots in every cell"""
    q = _seeded(ni, 20261021 + ni[0])
    PT2.advect_rk2(q, *_rotation(ni), 1.0)
    q, _, c = PT2.move(q)
    assert c["n_far"] == 0 and c["n_overflow"] == 0
    return q


# ---------------------------------------------------------------------------------------------- to the device and back
def _device_particles(jr, q, fields=()):
    """a device Particles holding the cloud q and its particle fields, and sentinels in everything a move or an injection writes"""
    ni = (q.nx, q.ny) if not hasattr(q, "nz") else (q.nx, q.ny, q.nz)
    if len(ni) == 2:
        p = jr.init_particles(jr.AMDGPUBackend, q.nxcell, q.max_xcell, q.min_xcell, _xvi(ni), ni)
    else:
        p = jr.init_particles(jr.AMDGPUBackend, q.nxcell, q.max_xcell, q.min_xcell, *_xi_vel(ni))
    ax = "xyz"[:len(ni)]
    names = [x + "0" for x in ax] + ["d" + x for x in ax] + ["_d" + x for x in ax]
    assert p.ni == ni and [getattr(p, k) for k in names] == [getattr(q, k) for k in names]
    for c, a in zip(p.coords, (q.px, q.py, getattr(q, "pz", None))):
        c.copy_(_up(a))
    p.index.copy_(_up_int(q.active))
    dev = jr.init_cell_arrays(p, len(fields)) if fields else ()
    for d, f in zip(dev, fields):
        d.copy_(_up(f))
        p._twins[id(d)][1].fill_(SENTINEL)
    for c in p._coords2:
        c.fill_(SENTINEL)
    p._index2.fill_(-77)
    if len(ni) == 3:
        p._work.fill_(99)
    return p, dev


def _host(jr, p):
    """the coordinates and the mask"""
    return tuple(jr.to_numpy(c) for c in p.coords) + (_host_int(p.index),)


def _assert_state(jr, p, dev, q, fields, what=""):
    *coords, act = _host(jr, p)
    assert _same(act, q.active), (what, "active", int((act != q.active).sum()))
    for name, got in zip(("px", "py", "pz"), coords):
        assert _same(got, getattr(q, name)), (what, name, _ndiff(got, getattr(q, name)))
    for k, (d, f) in enumerate(zip(dev, fields)):
        assert _same(jr.to_numpy(d), f), (what, "field", k)


def _assert_cloud_untouched(jr, p, q):
    _assert_state(jr, p, (), q, ())


def _move(jr, p, dev, h):
    """move_particles_ with the error of a lossy move turned back into its counts"""
    try:
        return jr.move_particles_(p, dev, handle=h), None
    except RuntimeError as e:
        return e.counts, str(e)
