"""Marker-in-cell particles on the device, 2D and (the core chain) 3D: init_particles, init_cell_arrays, RungeKutta2, advection!, move_particles!, grid2particle!, particle2grid! and
update_phase_ratios!(phase_ratios, particles, pPhases) -- the chain the reference's miniapps take from JustPIC (miniapps/benchmarks/stokes2D/shear_heating/
Shearheating2D.jl:69-82,221-232).  Julia's `f!` is spelled `f_`.  JustPIC's text is not in the reference tree: include/jrx.h holds the definitions of what is
built, tests/_particles2d.py restates them in NumPy.  Every operator forwards to one C-ABI entry point (csrc/particles.hip); only the seeding is computed
here, on the host.

The elastic stress travels on the particles too: centroid2particle_, particle2centroid_, rotate_stress_particles_, stress2grid_ and the particle form of
rotate_stress_ (the tuple methods of src/stress_rotation/stress_rotation_particles.jl:92-99,224-235,264-276; tests/_particles2d_stress.py restates them).

Built: uniform grid, one block, fp64.  2D: everything below.  3D (csrc/particles3d.hip, tests/_particles3d.py; the chain of Shearheating3D.jl:63-78,224-233):
init_particles(backend, nxcell, max_xcell, min_xcell, *grid.xi_vel), init_cell_arrays, advection_, move_particles_, grid2particle_, particle2grid_,
centroid2particle_, particle2centroid_ and update_phase_ratios_ (all eight members); these dispatch on len(particles.ni).  Refused by name: in 3D
inject_particles_phase_, the stress operators and subgrid diffusion (a flow that crosses the boundary loses material there; n_outside reports it); in any
dimension a non-uniform Geometry, a handle with a communicator (by the library), a marker chain, StressParticles (the wrapper type; its tuple methods are what
is built).

A time step with particles (examples/sinking_block2d_particles.py; with the refill, examples/rotating_box2d_injection.py):

    advection_(particles, RungeKutta2(), stokes.V, dt); move_particles_(particles, particle_args); inject_particles_phase_(particles, pPhases, args, fields);
    update_phase_ratios_(phase_ratios, particles, pPhases); compute_ρg_(...); solve_(...)

inject_particles_phase_ refills the cells that fell below min_xcell particles (operator 12 of include/jrx.h; tests/_particles2d_inject.py restates it): new
particles on the empty sites of the sub-cell lattice of init_particles, the phase from the nearest particle, the other fields from the grid or from that particle.

A visco-elastic step with the stress on particles (examples/stress_rotation2d_particles.py), pτxx, pτyy, pτxy, pω from init_cell_arrays:

    stress2grid_(stokes, pτxx, pτyy, pτxy, particles); solve_(...); compute_vorticity(stokes, di)
    rotate_stress_(pτxx, pτyy, pτxy, pω, stokes, particles, dt); advection_(...); move_particles_(particles, (pτxx, pτyy, pτxy, pω, ...))

A thermal step with the temperature on particles (examples/thermal_particles2d.py), subgrid_arrays = SubgridDiffusionCellArrays(particles, loc="center"):

    particle2centroid_(T, pT, particles); T_buffer = T; heatdiffusion_PT_(...); subgrid_characteristic_time_(dt0, ...)
    centroid2particle_(subgrid_arrays.dt0, dt0, particles); subgrid_diffusion_centroid_(pT, T_buffer, thermal.ΔT, subgrid_arrays, particles, dt)

(JustPIC's subgrid_diffusion_centroid! / subgrid_diffusion!, operators 10 and 11 of include/jrx.h; tests/_particles2d_subgrid.py restates them).

Layout: every per-particle array is (nx, ny[, nz], max_xcell) column-major, the slot index slowest; an inactive slot holds 0 in every array.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .arrays import from_numpy, fzeros, ptr
from .backend import device_of
from .gridops import _h
from .stress_rotation import METHODS
from .phases import _ULPS          # the vertex spacing may vary by this many ulp of the largest coordinate, as for update_phase_ratios_2D_

COUNTS = ("n_active_before", "n_active_after", "n_outside", "n_far", "n_overflow")
INJECT_COUNTS = ("n_active_before", "n_active_after", "n_deficient", "n_injected", "n_no_donor")
INJECT_LOCS = {"vertex": _lib.INJECT_VERTEX, "center": _lib.INJECT_CENTRE, "donor": _lib.INJECT_DONOR}


def _not_built(what):
    raise NotImplementedError(f"{what}: not built (particles are built for uniform grids and one block, the core chain in 2D and 3D, everything else in 2D; marker chains and StressParticles are not provided)")


def inject_particles_phase_(particles=None, pPhases=None, args=(), fields=(), *, loc=None, min_xcell=None, handle=None):
    """inject_particles_phase!(particles, pPhases, args, fields): every cell with fewer than min_xcell particles (default: particles.min_xcell) is refilled, one
    launch.  The new particles sit on the empty sites of the sub-cell lattice of init_particles (deterministic, where JustPIC draws them at random); each takes its
    phase from the nearest particle of its own and the eight neighbouring cells, and args[k] from fields[k]: a vertex field (nx+1, ny+1) or a centre field (nx, ny)
    interpolated at the new point, or None for the donor's value.  loc may name the kinds ("vertex", "center", "donor") and must agree with the shapes.  A particle
    field that is not listed keeps 0 in the new slots.  Returns the counters as a dict; a cell with no particle in its neighbourhood is counted in n_no_donor and
    heals in a later step (include/jrx.h, operator 12).  Call it after move_particles_."""
    fn = "inject_particles_phase!"
    if particles is None:
        _not_built(f"{fn} without particles")
    _check_particles(particles, fn)
    _check_field(particles, pPhases, "pPhases", fn)
    args, fields = tuple(args), tuple(fields)
    if len(args) != len(fields):
        raise ValueError(f"{fn}: {len(args)} particle fields and {len(fields)} grid fields (one per particle field; None copies the donor's value)")
    if len(args) > _lib.MAXPHASE:
        raise ValueError(f"{fn}: {len(args)} particle fields (0 .. {_lib.MAXPHASE})")
    loc = (None,) * len(args) if loc is None else tuple(loc)
    if len(loc) != len(args):
        raise ValueError(f"{fn}: loc names {len(loc)} kinds for {len(args)} particle fields")
    nx, ny = particles.ni
    shapes = {(nx + 1, ny + 1): "vertex", (nx, ny): "center"}
    codes = []
    for k, (f, F, want) in enumerate(zip(args, fields, loc)):
        _check_field(particles, f, f"args[{k}]", fn)
        if f is pPhases:
            raise ValueError(f"{fn}: args[{k}] is pPhases (the phases are carried by the operator itself)")
        want = want.lstrip(":") if isinstance(want, str) else want
        if want is not None and want not in INJECT_LOCS:
            raise ValueError(f"{fn}: unknown loc[{k}] = {want!r} (one of {sorted(INJECT_LOCS)})")
        if F is None:
            kind = "donor"
        elif isinstance(F, torch.Tensor) and F.dtype == torch.float64 and tuple(F.shape) in shapes:
            kind = shapes[tuple(F.shape)]
            if F.device != particles.coords[0].device:
                raise ValueError(f"{fn}: fields[{k}] is on {F.device}, the particles on {particles.coords[0].device}")
        else:
            raise ValueError(f"{fn}: fields[{k}] is {tuple(F.shape) if isinstance(F, torch.Tensor) else type(F).__name__}; {particles.ni} cells need an fp64 vertex "
                             f"field {(nx + 1, ny + 1)}, a centre field {(nx, ny)} or None (the donor's value)")
        if want is not None and want != kind:
            raise ValueError(f"{fn}: loc[{k}] = {want!r}, but fields[{k}] is {'None' if F is None else tuple(F.shape)}: a {kind} field")
        if kind == "center" and min(particles.ni) < 2:
            raise ValueError(f"{fn}: {particles.ni} cells (interpolation between centres needs nx >= 2 and ny >= 2)")
        codes.append(INJECT_LOCS[kind])
    if len({id(f) for f in args}) != len(args):
        raise ValueError(f"{fn}: a particle field is listed twice")
    min_xcell = particles.min_xcell if min_xcell is None else int(min_xcell)
    nsx, nsy = _lattice(particles.nxcell)
    if not 1 <= min_xcell <= min(particles.max_xcell, nsx * nsy):
        raise ValueError(f"{fn}: min_xcell = {min_xcell} (must lie in 1 .. min(max_xcell = {particles.max_xcell}, nxcell = {nsx * nsy}))")
    if nsx * nsy > 64:
        raise ValueError(f"{fn}: nxcell = {nsx * nsy} (the lattice of new sites holds 64 at the most)")
    h = _h(particles.coords[0], handle)
    n = len(args)
    s = particles._struct()
    a_args = (C.c_void_p * max(n, 1))(*(ptr(f) for f in args))
    a_fields = (C.c_void_p * max(n, 1))(*(None if F is None else ptr(F) for F in fields))
    a_loc = (C.c_int32 * max(n, 1))(*codes)
    counts = (C.c_int64 * 5)()
    h.call("jrx_particles2d_inject", C.byref(s), C.c_void_p(particles._index2.data_ptr()), C.c_void_p(ptr(pPhases)), a_args, a_fields, a_loc, C.c_int32(n),
           C.c_int32(min_xcell), C.c_int32(nsx), C.c_int32(nsy), counts)
    particles.index, particles._index2 = particles._index2, particles.index          # the mask was written out of place
    return dict(zip(INJECT_COUNTS, (int(c) for c in counts)))


def MarkerChain(*a, **k):
    _not_built("MarkerChain")


def StressParticles(*a, **k):
    _not_built("StressParticles")


class RungeKutta2:
    """RungeKutta2(): the midpoint rule (α = 0.5), the only member of the family that is built"""

    def __init__(self, α=0.5):
        if float(α) != 0.5:
            raise NotImplementedError(f"RungeKutta2(α = {α}): only the midpoint rule α = 0.5 is built")
        self.α = 0.5


def _lattice(nxcell):
    nsx = max(d for d in range(1, int(np.floor(np.sqrt(nxcell))) + 1) if nxcell % d == 0)
    return nsx, nxcell // nsx


def _lattice3(nxcell):
    """(nsx, nsy, nsz) of the 3D seeding lattice: nsx the largest divisor of nxcell with nsx^3 <= nxcell, nsy the largest divisor of the rest with nsy^2 <= rest"""
    nsx = max(d for d in range(1, nxcell + 1) if nxcell % d == 0 and d * d * d <= nxcell)
    rest = nxcell // nsx
    nsy = max(d for d in range(1, rest + 1) if rest % d == 0 and d * d <= rest)
    return nsx, nsy, rest // nsy


def _izeros(shape, device):
    t = torch.zeros(tuple(shape)[::-1], dtype=torch.int32, device=device)
    return t.permute(*range(len(shape) - 1, -1, -1))


class Particles:
    """What init_particles returns: coords = (px, py[, pz]) and index (the int32 mask `active`), each (nx, ny[, nz], max_xcell); the grid (x0, y0[, z0], dx, dy[, dz]
    and the inverses formed once here); a second set of buffers for the out-of-place move, and one twin per particle field of init_cell_arrays.  3D particles also
    own the byte buffer of the move (one byte per slot: include/jrx.h, jrx_particles3d_move)."""

    def __init__(self, device, ni, max_xcell, min_xcell, nxcell, origin, spacing):
        self.ni, self.max_xcell, self.min_xcell, self.nxcell = tuple(ni), int(max_xcell), int(min_xcell), int(nxcell)
        nd = len(self.ni)
        self.origin, self.di = tuple(float(v) for v in origin), tuple(float(v) for v in spacing)
        self._di = tuple(1.0 / v for v in self.di)
        for axis, c in enumerate("xyz"[:nd]):
            setattr(self, c + "0", self.origin[axis]), setattr(self, "d" + c, self.di[axis]), setattr(self, "_d" + c, self._di[axis])
        shape = self.ni + (self.max_xcell,)
        self.device = device
        self.coords = tuple(fzeros(shape, device) for _ in range(nd))
        self.index = _izeros(shape, device)
        self._coords2 = tuple(fzeros(shape, device) for _ in range(nd))
        self._index2 = _izeros(shape, device)
        self._twins = {}          # id(particle field) -> (field, twin)
        self._work = torch.zeros(int(np.prod(shape)), dtype=torch.uint8, device=device) if nd == 3 else None

    @property
    def shape(self):
        return self.ni + (self.max_xcell,)

    def _struct(self, second=False):
        coords = self._coords2 if second else self.coords
        idx = self._index2 if second else self.index
        cls = _lib.Particles2D if len(self.ni) == 2 else _lib.Particles3D
        return cls(*(ptr(c) for c in coords), idx.data_ptr(), *self.ni, self.max_xcell, *self.origin, *self.di, *self._di)

    def _swap(self, fields):
        self.coords, self._coords2 = self._coords2, self.coords
        self.index, self._index2 = self._index2, self.index
        for f in fields:          # the caller's tensor object keeps its identity and takes the storage that was just written
            twin = self._twins[id(f)][1]
            f.data, twin.data = twin.data, f.data


def _uniform_vertices(xvi, ni, fn, dims=(2,)):
    if hasattr(xvi, "xvi"):          # a Geometry
        if getattr(xvi, "nonuniform", False):
            raise NotImplementedError(f"{fn}: a non-uniform Geometry (particles are built for uniform grids)")
        xvi = xvi.xvi
    ni = tuple(int(n) for n in ni)
    if len(ni) not in dims or len(xvi) != len(ni):
        raise NotImplementedError(f"{fn}: {len(ni)}D extents with {len(xvi)} vertex vectors (this form, (xvi, ni), is built in 2D; 3D particles come from "
                                  f"{fn}(backend, nxcell, max_xcell, min_xcell, *grid.xi_vel))")
    if any(n < 1 for n in ni):
        raise ValueError(f"{fn}: ni = {ni}")
    xv = [np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64) for x in xvi]
    for d in range(len(ni)):
        if xv[d].shape != (ni[d] + 1,):
            raise ValueError(f"{fn}: dimension {d + 1} has {ni[d]} cells, xvi[{d}] has {xv[d].size} entries (expected {ni[d] + 1})")
        steps = np.diff(xv[d])
        if not np.all(np.isfinite(xv[d])) or not steps[0] > 0.0 or not np.all(np.abs(steps - steps[0]) <= _ULPS * np.spacing(np.abs(xv[d]).max())):
            raise NotImplementedError(f"{fn}: the vertices of dimension {d + 1} are not uniform (particles are built for uniform grids)")
    return ni, xv


def init_particles(backend_tag, nxcell, max_xcell, min_xcell, *grids, rng=None):
    """init_particles(backend, nxcell, max_xcell, min_xcell, grid.xi_vel...) -- the reference's call shape, two velocity grids for 2D and three for 3D: the vertex
    vector of axis d is xi_vel[d][d] -- or, in 2D, init_particles(backend, nxcell, max_xcell, min_xcell, xvi, ni) with the two vertex vectors (or a Geometry) and
    the extents; both give the same particles.  nxcell particles per cell in slots 0 .. nxcell - 1 on a regular sub-cell lattice.  2D: nsx x nsy, nsx the largest
    divisor of nxcell not above its square root, slot s = a + nsx b at (x0 + i dx) + (a + u) dx / nsx, (y0 + j dy) + (b + v) dy / nsy.  3D: nsx x nsy x nsz, nsx the
    largest divisor with nsx^3 <= nxcell, nsy the largest divisor of the rest r = nxcell / nsx with nsy^2 <= r, nsz = r / nsy (8: 2 2 2; 20: 2 2 5), slot
    s = a + nsx (b + nsy c).  u = v = w = 0.5; with rng, a NumPy Generator, 0.05 + 0.9 r with r = rng.random(ni + (nxcell,)), drawn for x, then y, then z:
    jittered inside the sub-cell.  Built on the host, so the same arguments give the same particles."""
    fn = "init_particles"
    if len(grids) == 2 and (hasattr(grids[0], "xvi") or all(isinstance(n, (int, np.integer)) for n in grids[1])):
        ni, xv = _uniform_vertices(grids[0], grids[1], fn)
    elif len(grids) in (2, 3) and all(not hasattr(g, "xvi") and len(g) == len(grids) for g in grids):
        xvi = tuple(grids[d][d] for d in range(len(grids)))
        ni, xv = _uniform_vertices(xvi, tuple(len(x) - 1 for x in xvi), fn, dims=(2, 3))
    else:
        raise TypeError(f"{fn}: expected (xvi, ni) or the {len(grids)} velocity grids grid.xi_vel..., each with {len(grids)} coordinate vectors")
    nd = len(ni)
    nxcell, max_xcell, min_xcell = int(nxcell), int(max_xcell), int(min_xcell)
    if not 0 <= min_xcell <= nxcell <= max_xcell or nxcell < 1:
        raise ValueError(f"{fn}: need 0 <= min_xcell <= nxcell <= max_xcell and nxcell >= 1, got nxcell = {nxcell}, max_xcell = {max_xcell}, min_xcell = {min_xcell}")
    if int(np.prod(ni, dtype=object)) * max_xcell >= 2 ** 31:
        raise ValueError(f"{fn}: {' x '.join(str(n) for n in ni)} x {max_xcell} slots: 2^31 or more (32-bit offsets)")
    dev = device_of(backend_tag)
    origin, spacing = [float(x[0]) for x in xv], [float(x[1] - x[0]) for x in xv]
    ns = _lattice(nxcell) if nd == 2 else _lattice3(nxcell)
    s = np.arange(nxcell)
    sub = [s % ns[0], s // ns[0]] if nd == 2 else [s % ns[0], (s // ns[0]) % ns[1], s // (ns[0] * ns[1])]
    shape = ni + (nxcell,)
    jitter = [np.full(shape, 0.5) if rng is None else 0.05 + 0.9 * rng.random(shape) for _ in range(nd)]
    p = Particles(dev, ni, max_xcell, min_xcell, nxcell, origin, spacing)
    for d in range(nd):
        cell = (origin[d] + np.arange(ni[d], dtype=np.float64) * spacing[d]).reshape([-1 if q == d else 1 for q in range(nd + 1)])
        c = np.zeros(ni + (max_xcell,))
        c[..., :nxcell] = cell + (sub[d].astype(np.float64).reshape((1,) * nd + (-1,)) + jitter[d]) * (spacing[d] / ns[d])
        p.coords[d].copy_(from_numpy(c, dev))
    p.index[..., :nxcell] = 1
    return p


def init_cell_arrays(particles, n):
    """init_cell_arrays(particles, Val(n)): n particle fields (nx, ny[, nz], max_xcell), zero; each gets a twin for the out-of-place move"""
    n = int(n)
    if not 1 <= n <= _lib.MAXPHASE:
        raise ValueError(f"init_cell_arrays: {n} particle fields (1 .. {_lib.MAXPHASE})")
    out = []
    for _ in range(n):
        f, twin = fzeros(particles.shape, particles.device), fzeros(particles.shape, particles.device)
        particles._twins[id(f)] = (f, twin)
        out.append(f)
    return tuple(out)


def _check_particles(particles, fn, dims=(2,)):
    """dims: the dimensions this operator is built in; 3D particles are refused by name before anything reaches the device"""
    if not isinstance(particles, Particles):
        raise TypeError(f"{fn}: particles must come from init_particles, got {type(particles).__name__}")
    if len(particles.ni) not in dims:
        raise NotImplementedError(f"{fn}: {len(particles.ni)}D particles ({' and '.join(f'{d}D' for d in dims)} {'are' if len(dims) > 1 else 'is'} built"
                                  f"{'; in 3D: advect, move, the four interpolations and the phase ratios' if len(particles.ni) == 3 else ''})")


def _check_field(particles, f, name, fn):
    if not isinstance(f, torch.Tensor) or f.dtype != torch.float64 or tuple(f.shape) != particles.shape:
        raise ValueError(f"{fn}: {name} must be an fp64 array of {particles.shape} (init_cell_arrays), got "
                         f"{tuple(f.shape) if isinstance(f, torch.Tensor) else type(f).__name__}")
    if f.device != particles.coords[0].device:
        raise ValueError(f"{fn}: {name} is on {f.device}, the particles on {particles.coords[0].device}")


def _check_grid(particles, grid, fn):
    """a Geometry handed along is the particles' grid"""
    if grid is None:
        return
    if getattr(grid, "nonuniform", False):
        raise NotImplementedError(f"{fn}: a non-uniform Geometry (particles are built for uniform grids)")
    if len(grid.ni) != len(particles.ni):
        raise NotImplementedError(f"{fn}: a {len(grid.ni)}D grid " + ("(particles are built in 2D)" if len(particles.ni) == 2 else "with 3D particles"))
    if tuple(grid.ni) != particles.ni:
        raise ValueError(f"{fn}: the grid has {tuple(grid.ni)} cells, the particles {particles.ni}")


def advection_(particles, method, V, dt, *, grid=None, handle=None):
    """advection!(particles, RungeKutta2(), @velocity(stokes), dt): every particle by the midpoint rule through the bilinear (3D: trilinear) interpolant of
    V = stokes.V (or the tuple of its components, ghost layers included), in place (include/jrx.h, jrx_particles2d_advect_rk2 / jrx_particles3d_advect_rk2).
    Follow it with move_particles_."""
    fn = "advection!"
    _check_particles(particles, fn, (2, 3))
    if not isinstance(method, RungeKutta2):
        raise NotImplementedError(f"{fn}: {type(method).__name__} (RungeKutta2() is built)")
    _check_grid(particles, grid, fn)
    nd = len(particles.ni)
    Vs = tuple(getattr(V, k) for k in ("Vx", "Vy", "Vz") if getattr(V, k, None) is not None) if hasattr(V, "Vx") else tuple(V)
    if len(Vs) != nd or any(v.dim() != nd for v in Vs):
        raise NotImplementedError(f"{fn}: V has {len(Vs)} components of {[v.dim() for v in Vs]} dimensions ({nd}D particles need {nd} components of {nd} dimensions)")
    want = tuple(tuple(n + (1 if a == d else 2) for a, n in enumerate(particles.ni)) for d in range(nd))
    if tuple(tuple(v.shape) for v in Vs) != want:
        raise ValueError(f"{fn}: V is {', '.join(str(tuple(v.shape)) for v in Vs)}; {particles.ni} cells need {', '.join(str(w) for w in want)}")
    h = _h(particles.coords[0], handle)
    for k, v in zip(("V.Vx", "V.Vy", "V.Vz"), Vs):
        if v.device != particles.coords[0].device:
            raise ValueError(f"{fn}: {k} is on {v.device}, the particles on {particles.coords[0].device}")
    s = particles._struct()
    h.call(f"jrx_particles{nd}d_advect_rk2", C.byref(s), *(C.c_void_p(ptr(v)) for v in Vs), C.c_double(float(dt)))


def move_particles_(particles, particle_args=(), *, handle=None):
    """move_particles!(particles, particle_args): every particle into the bucket of the cell that owns its coordinate, particle_args (fields of init_cell_arrays)
    along with it; out of place into the second set of buffers, which then becomes the current one (the tensors of particle_args keep their identity).  Returns the
    counters as a dict.  RuntimeError naming the counter when particles were lost to a full bucket (n_overflow) or to a jump of more than one cell (n_far): the state
    is then valid, without those particles.  Particles that left the grid (n_outside) are dropped silently, as the count says."""
    fn = "move_particles!"
    _check_particles(particles, fn, (2, 3))
    args = tuple(particle_args)
    if len(args) > _lib.MAXPHASE:
        raise ValueError(f"{fn}: {len(args)} particle fields (0 .. {_lib.MAXPHASE})")
    for k, f in enumerate(args):
        _check_field(particles, f, f"particle_args[{k}]", fn)
        if id(f) not in particles._twins:
            raise ValueError(f"{fn}: particle_args[{k}] does not come from init_cell_arrays of these particles (it has no twin to move into)")
    if len({id(f) for f in args}) != len(args):
        raise ValueError(f"{fn}: a particle field is listed twice")
    h = _h(particles.coords[0], handle)
    n = len(args)
    src, dst = particles._struct(), particles._struct(second=True)
    a_src = (C.c_void_p * max(n, 1))(*(ptr(f) for f in args))
    a_dst = (C.c_void_p * max(n, 1))(*(ptr(particles._twins[id(f)][1]) for f in args))
    counts = (C.c_int64 * 5)()
    if len(particles.ni) == 2:
        h.call("jrx_particles2d_move", C.byref(src), C.byref(dst), a_src, a_dst, C.c_int32(n), counts)
    else:          # the particles' byte buffer: the library stores every slot's owner in it (tuning key particles3d_move_codes = 0: the direct form)
        h.call("jrx_particles3d_move", C.byref(src), C.byref(dst), a_src, a_dst, C.c_int32(n), C.c_void_p(particles._work.data_ptr()), counts)
    particles._swap(args)
    out = dict(zip(COUNTS, (int(c) for c in counts)))
    for k in ("n_far", "n_overflow"):
        if out[k]:
            err = RuntimeError(f"{fn}: {k} = {out[k]} particles were lost ({'they moved more than one cell: reduce dt' if k == 'n_far' else 'their cell is full: raise max_xcell'}); "
                               f"counts = {out}")
            err.counts = out
            raise err
    return out


def _field_op(entry, first, second, F, pF, kind, particles, handle):
    """operators 3, 4, 6, 7: one particle field pF and one grid field F on the vertices or the centres; `first` is the one written"""
    fn = entry + "!"
    _check_particles(particles, fn, (2, 3))
    _check_field(particles, pF, "pF", fn)
    _check_grid_field(particles, F, "F", tuple(n + 1 for n in particles.ni) if kind == "vertex" else particles.ni, kind, fn)
    if entry == "centroid2particle" and min(particles.ni) < 2:
        raise ValueError(f"{fn}: {particles.ni} cells (interpolation between centres needs {'nx >= 2 and ny >= 2' if len(particles.ni) == 2 else 'every extent >= 2'})")
    h = _h(pF, handle)
    s = particles._struct()
    h.call(f"jrx_particles{len(particles.ni)}d_{entry}", C.c_void_p(ptr(first)), C.c_void_p(ptr(second)), C.byref(s))


def grid2particle_(pF, F, particles, *, handle=None):
    """grid2particle!(pF, xvi, F, particles): the vertex field F (nx+1, ny+1[, nz+1]) to the particles, bilinear (trilinear) in the cell of each particle's bucket"""
    _field_op("grid2particle", pF, F, F, pF, "vertex", particles, handle)


def particle2grid_(F, pF, particles, *, handle=None):
    """particle2grid!(F, pF, xvi, particles): the particle field pF to the vertex field F (nx+1, ny+1[, nz+1]), weighted by the bilinear (trilinear) distance of
    each particle of the up to four (eight) cells around a vertex; a vertex without a particle around it keeps its value"""
    _field_op("particle2grid", F, pF, F, pF, "vertex", particles, handle)


def update_phase_ratios_(phase_ratios, particles, pPhases, *, handle=None):
    """update_phase_ratios!(phase_ratios, particles, pPhases): center, vertex, Vx and Vy (3D: and Vz, yz, xz, xy) of phase_ratios from the phases 1.0 .. N of the
    particles, one launch.  Returns n_empty, the number of (node, member) pairs no particle weight reached (left unchanged)."""
    fn = "update_phase_ratios!"
    _check_particles(particles, fn, (2, 3))
    _check_field(particles, pPhases, "pPhases", fn)
    N = int(phase_ratios.nphases)
    if not 1 <= N <= _lib.MAXPHASE:
        raise ValueError(f"{fn}: {N} phases (1 .. {_lib.MAXPHASE})")
    nd = len(particles.ni)
    if phase_ratios.center.dim() != nd + 1:
        raise NotImplementedError(f"{fn}: a {phase_ratios.center.dim() - 1}D PhaseRatios " + ("(2D is built)" if nd == 2 else "with 3D particles"))
    stag = dict(center=(0, 0), vertex=(1, 1), Vx=(1, 0), Vy=(0, 1)) if nd == 2 else \
        dict(center=(0, 0, 0), vertex=(1, 1, 1), Vx=(1, 0, 0), Vy=(0, 1, 0), Vz=(0, 0, 1), yz=(0, 1, 1), xz=(1, 0, 1), xy=(1, 1, 0))
    want = {k: (N,) + tuple(n + s for n, s in zip(particles.ni, st)) for k, st in stag.items()}
    for k, shp in want.items():
        m = getattr(phase_ratios, k, None)
        if m is None or tuple(m.shape) != shp:
            raise ValueError(f"{fn}: phase_ratios.{k} is {None if m is None else tuple(m.shape)}, the particles {particles.ni} need {shp}")
    h = _h(pPhases, handle)
    if phase_ratios.center.device != pPhases.device:
        raise ValueError(f"{fn}: phase_ratios is on {phase_ratios.center.device}, pPhases on {pPhases.device}")
    s = particles._struct()
    n_empty = C.c_int64()
    if nd == 2:
        h.call("jrx_particles2d_phase_ratios", *(C.c_void_p(ptr(getattr(phase_ratios, k))) for k in want), C.c_void_p(ptr(pPhases)), C.c_int32(N), C.byref(s),
               C.byref(n_empty))
    else:
        h.call("jrx_particles3d_phase_ratios", _vec([getattr(phase_ratios, k) for k in want]), C.c_void_p(ptr(pPhases)), C.c_int32(N), C.byref(s), C.byref(n_empty))
    return int(n_empty.value)


# ---------------------------------------------------------------------------------------------- the elastic stress on particles
def _check_grid_field(particles, F, name, shape, kind, fn):
    if not isinstance(F, torch.Tensor) or F.dtype != torch.float64 or tuple(F.shape) != shape:
        raise ValueError(f"{fn}: {name} is {tuple(F.shape) if isinstance(F, torch.Tensor) else type(F).__name__}; {particles.ni} cells need the {kind} field {shape}")
    if F.device != particles.coords[0].device:
        raise ValueError(f"{fn}: {name} is on {F.device}, the particles on {particles.coords[0].device}")


def _method(method, fn):
    m = method.lstrip(":") if isinstance(method, str) else method
    if m not in METHODS:
        raise ValueError(f"{fn}: unknown method {method!r} (one of {sorted(METHODS)})")
    return C.c_int32(METHODS[m])


def _check_stokes(particles, stokes, fn):
    ni = getattr(stokes, "_ni", None)
    if ni is None or not hasattr(stokes, "τ_o"):
        raise TypeError(f"{fn}: stokes must be a StokesArrays, got {type(stokes).__name__}")
    if len(ni) != 2:
        raise NotImplementedError(f"{fn}: a {len(ni)}D StokesArrays (particles are built in 2D)")
    if tuple(ni) != particles.ni:
        raise ValueError(f"{fn}: stokes has {tuple(ni)} cells, the particles {particles.ni}")
    if stokes.P.device != particles.coords[0].device:
        raise ValueError(f"{fn}: stokes is on {stokes.P.device}, the particles on {particles.coords[0].device}")


def _vec(ts):
    return (C.c_void_p * len(ts))(*(ptr(t) for t in ts))


def centroid2particle_(pF, F, particles, *, handle=None):
    """centroid2particle!(pF, F, particles): the centre field F (nx, ny[, nz]) to the particles, bilinear (trilinear) between the four (eight) centres around each
    particle's coordinate; a particle in the outer half cells extrapolates from the outermost pair.  Needs every extent >= 2 (include/jrx.h, operator 6)."""
    _field_op("centroid2particle", pF, F, F, pF, "centre", particles, handle)


def particle2centroid_(F, pF, particles, *, handle=None):
    """particle2centroid!(F, pF, particles): the particle field pF to the centre field F (nx, ny[, nz]), each cell from its own bucket weighted by the bilinear
    (trilinear) distance to the centre; a cell without a particle keeps its value (operator 7)"""
    _field_op("particle2centroid", F, pF, F, pF, "centre", particles, handle)


def _stress_fields(particles, pτ, fn):
    pτ = tuple(pτ)
    if len(pτ) != 3:
        raise NotImplementedError(f"{fn}: {len(pτ)} stress components (2D is built: pτxx, pτyy, pτxy)")
    for name, f in zip(("pτxx", "pτyy", "pτxy"), pτ):
        _check_field(particles, f, name, fn)
    return pτ


def rotate_stress_particles_(pτ, pω, particles, dt, *, method="matrix", handle=None):
    """rotate_stress_particles!((pτxx, pτyy, pτxy), (pω,), particles, dt; method = :matrix): every particle's stress rotated in place by θ = dt pω, with the
    rotation matrix ("matrix") or the corrected Jaumann rate ("jaumann") of rotate_stress_ on grids (operator 8)"""
    fn = "rotate_stress_particles!"
    _check_particles(particles, fn)
    pτ = _stress_fields(particles, pτ, fn)
    pω = (pω,) if isinstance(pω, torch.Tensor) else tuple(pω)
    if len(pω) != 1:
        raise NotImplementedError(f"{fn}: {len(pω)} vorticity components (2D is built: one)")
    _check_field(particles, pω[0], "pω", fn)
    m = _method(method, fn)
    h = _h(pτ[0], handle)
    s = particles._struct()
    h.call("jrx_particles2d_rotate", _vec(pτ), C.c_void_p(ptr(pω[0])), C.byref(s), C.c_double(float(dt)), m)


def _rotate_stress_particles_form(pτxx, pτyy, pτxy, pω, stokes, particles, dt, *, method="matrix", handle=None):
    """the particle form of rotate_stress_ (stress_rotation.py dispatches here): stokes.τ.xx, τ.yy (centres) and τ.xy, ω.xy (vertices) to the particles, then the
    rotation of rotate_stress_particles_; one launch (operator 9)"""
    fn = "rotate_stress!"
    _check_particles(particles, fn)
    pτ = _stress_fields(particles, (pτxx, pτyy, pτxy), fn)
    _check_field(particles, pω, "pω", fn)
    _check_stokes(particles, stokes, fn)
    if min(particles.ni) < 2:
        raise ValueError(f"{fn}: {particles.ni} cells (interpolation between centres needs nx >= 2 and ny >= 2)")
    m = _method(method, fn)
    h = _h(pτ[0], handle)
    s = particles._struct()
    τ = stokes.τ
    h.call("jrx_particles2d_rotate_stress", _vec(pτ), C.c_void_p(ptr(pω)), C.c_void_p(ptr(τ.xx)), C.c_void_p(ptr(τ.yy)), C.c_void_p(ptr(τ.xy)),
           C.c_void_p(ptr(stokes.ω.xy)), C.byref(s), C.c_double(float(dt)), m)


def stress2grid_(stokes, pτxx, pτyy, pτxy, particles, *, handle=None):
    """stress2grid!(stokes, pτxx, pτyy, pτxy, particles): stokes.τ_o.xx, yy, xy_c (centres, particle2centroid_) and τ_o.xx_v, yy_v, xy (vertices, particle2grid_)
    from the particle stress, one launch; a node no particle weight reaches keeps its value (operator 9).  τ_o.xx_v, yy_v are allocated on first touch."""
    fn = "stress2grid!"
    _check_particles(particles, fn)
    pτ = _stress_fields(particles, (pτxx, pτyy, pτxy), fn)
    _check_stokes(particles, stokes, fn)
    h = _h(pτ[0], handle)
    s = particles._struct()
    τ_o = stokes.τ_o
    h.call("jrx_particles2d_stress2grid", _vec([τ_o.xx, τ_o.yy, τ_o.xy_c, τ_o.xy, τ_o.xx_v, τ_o.yy_v]), _vec(pτ), C.byref(s))


# ---------------------------------------------------------------------------------------------- the temperature on particles
SUBGRID_LOCS = ("vertex", "center")


class SubgridDiffusionCellArrays:
    """SubgridDiffusionCellArrays(particles; loc = :vertex): the scratch of subgrid_diffusion_ (loc "vertex") or subgrid_diffusion_centroid_ (loc "center") --
    pT0, pΔT and dt0 (the reference's dt₀: Python takes no subscript digit in a name) of the particle shape, ΔT_subgrid (nx, ny) for "center" and (nx+1, ny+1) for
    "vertex".  They are refilled in every step and get no twins: none of them travels with move_particles_."""

    def __init__(self, particles, loc="vertex"):
        fn = "SubgridDiffusionCellArrays"
        _check_particles(particles, fn)
        loc = loc.lstrip(":") if isinstance(loc, str) else loc
        if loc not in SUBGRID_LOCS:
            raise ValueError(f"{fn}: unknown loc {loc!r} (one of {SUBGRID_LOCS})")
        self.loc, self.ni = loc, particles.ni
        nx, ny = particles.ni
        self.pT0, self.pΔT, self.dt0 = (fzeros(particles.shape, particles.device) for _ in range(3))
        self.ΔT_subgrid = fzeros((nx, ny) if loc == "center" else (nx + 1, ny + 1), particles.device)


def _subgrid(fn, loc, pT, T_grid, ΔT_grid, subgrid_arrays, particles, dt, d, handle):
    _check_particles(particles, fn)
    if not isinstance(subgrid_arrays, SubgridDiffusionCellArrays):
        raise TypeError(f"{fn}: subgrid_arrays must be a SubgridDiffusionCellArrays, got {type(subgrid_arrays).__name__}")
    if subgrid_arrays.loc != loc:
        other = "subgrid_diffusion!" if loc == "center" else "subgrid_diffusion_centroid!"
        raise ValueError(f"{fn}: subgrid_arrays has loc = {subgrid_arrays.loc!r}, this operator needs {loc!r} ({other} takes {subgrid_arrays.loc!r})")
    if subgrid_arrays.ni != particles.ni:
        raise ValueError(f"{fn}: subgrid_arrays was made for {subgrid_arrays.ni} cells, the particles have {particles.ni}")
    sa = subgrid_arrays
    _check_field(particles, pT, "pT", fn)
    for name in ("pT0", "pΔT", "dt0"):
        _check_field(particles, getattr(sa, name), f"subgrid_arrays.{name}", fn)
    nx, ny = particles.ni
    kind, ext = ("centre", (nx, ny)) if loc == "center" else ("vertex", (nx + 1, ny + 1))
    _check_grid_field(particles, T_grid, "T_grid", ext, kind, fn)
    _check_grid_field(particles, sa.ΔT_subgrid, "subgrid_arrays.ΔT_subgrid", ext, kind, fn)
    ghosted = (ext[0] + 2, ext[1] + 2)
    if not isinstance(ΔT_grid, torch.Tensor) or ΔT_grid.dtype != torch.float64 or tuple(ΔT_grid.shape) not in (ext, ghosted):
        raise ValueError(f"{fn}: ΔT_grid is {tuple(ΔT_grid.shape) if isinstance(ΔT_grid, torch.Tensor) else type(ΔT_grid).__name__}; {particles.ni} cells need the "
                         f"{kind} field {ext} or, with its ghost layer (thermal.ΔT), {ghosted}")
    if ΔT_grid.device != particles.coords[0].device:
        raise ValueError(f"{fn}: ΔT_grid is on {ΔT_grid.device}, the particles on {particles.coords[0].device}")
    if loc == "center" and min(particles.ni) < 2:
        raise ValueError(f"{fn}: {particles.ni} cells (interpolation between centres needs nx >= 2 and ny >= 2)")
    d, dt = float(d), float(dt)
    if not 0.0 <= d <= 1.0:
        raise ValueError(f"{fn}: d = {d} (must lie in [0, 1])")
    if not (np.isfinite(dt) and dt >= 0.0):
        raise ValueError(f"{fn}: dt = {dt} (must be finite and not negative)")
    h = _h(pT, handle)
    s = particles._struct()
    code = _lib.SUBGRID_DT_GHOSTED if tuple(ΔT_grid.shape) == ghosted else _lib.SUBGRID_DT_NODES
    h.call("jrx_particles2d_subgrid_diffusion_centroid" if loc == "center" else "jrx_particles2d_subgrid_diffusion_vertex", C.c_void_p(ptr(pT)),
           C.c_void_p(ptr(T_grid)), C.c_void_p(ptr(ΔT_grid)), C.c_int32(code), C.c_void_p(ptr(sa.pT0)), C.c_void_p(ptr(sa.pΔT)), C.c_void_p(ptr(sa.dt0)),
           C.c_void_p(ptr(sa.ΔT_subgrid)), C.byref(s), C.c_double(d), C.c_double(dt))


def subgrid_diffusion_centroid_(pT, T_grid, ΔT_grid, subgrid_arrays, particles, dt, *, d=1.0, handle=None):
    """subgrid_diffusion_centroid!(pT, T_buffer, thermal.ΔT, subgrid_arrays, particles, dt; d = 1.0): the particle temperature pT takes the grid's diffusion step --
    the part of its difference to the grid temperature T_grid (centres, BEFORE the solve) that decays within dt at the particle's own rate subgrid_arrays.dt0
    (subgrid_characteristic_time_, then centroid2particle_(subgrid_arrays.dt0, dt0, particles): the caller's two steps), and the remainder of the grid's change
    ΔT_grid, (nx, ny) or thermal.ΔT itself (nx+2, ny+2), interpolated back; d = 0 adds the interpolated ΔT_grid only.  Two launches (include/jrx.h, operator 10)."""
    _subgrid("subgrid_diffusion_centroid!", "center", pT, T_grid, ΔT_grid, subgrid_arrays, particles, dt, d, handle)


def subgrid_diffusion_(pT, T_grid, ΔT_grid, subgrid_arrays, particles, dt, *, d=1.0, handle=None):
    """subgrid_diffusion!(pT, T_grid, ΔT_grid, subgrid_arrays, particles, dt; d = 1.0) with subgrid_arrays of loc "vertex": as subgrid_diffusion_centroid_ with the
    vertex fields T_grid, ΔT_grid (nx+1, ny+1), grid2particle_ / particle2grid_ in place of the centre operators.  Three launches (operator 11)."""
    _subgrid("subgrid_diffusion!", "vertex", pT, T_grid, ΔT_grid, subgrid_arrays, particles, dt, d, handle)
