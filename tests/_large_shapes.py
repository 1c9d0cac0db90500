"""Shape arithmetic for tests/test_gpu_large_offsets.py (pure Python, no GPU, no torch).

The hot kernels address with 32-bit byte offsets on uniform base pointers: `(const char *)p + u32 off`.  The upper half of
that range -- byte offsets from 2^31 to 2^32 -- only runs on blocks whose arrays are larger than 2 GiB.  This module names the shapes the GPU
tests use to get there, and computes from their extents which side of each size guard they fall on, where each staggered family's byte
offset crosses 2^31, the device memory a test holds, and the boxes and influence regions of the translated-blob check.  The CPU test
tests/test_large_offset_shapes.py pins all of it, so the shapes cannot drift out of the range they exist to test."""
from __future__ import annotations

GiB = 1 << 30
MiB = 1 << 20
F64 = 8
OFF31 = 1 << 31                # the upper half of the u32 byte-offset range starts here
HIGH_HALF_MIN = 2 * GiB + 64 * MiB

# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
# 3D Stokes and 3D VEP: every array (even the smallest, the residual Ry) is above 2 GiB + 64 MiB and below 4 GiB; nx > 384 and nz >= 384, so the
# 512-wide sweep tiles, the 64 x 8 fused tile and KZ = 12 are chosen; no extent is a multiple of a tile width
HIGH3 = (770, 598, 610)
# 2D: just below the 2^29-node guard of the one-launch batch form k_fused2d_b (byte offsets close to 4 GiB) and just above it
BELOW2 = (23000, 23000)
ABOVE2 = (23200, 23200)
# the small grids of the translated-blob check
SMALL3 = (64, 64, 64)
SMALL2 = (64, 64)

# ---- the guards (csrc) -------------------------------------------------------------------------------------------------------------


def fits_u32(ni):
    """stokes3d.hip fits_u32: the z-marching sweeps and the fused PT kernel run only when (nx+2)(ny+2)(nz+2) * 8 < 4 GiB"""
    nx, ny, nz = ni
    return (nx + 2) * (ny + 2) * (nz + 2) * F64 < 1 << 32


def vep3_accepts(ni):
    """stokes3d_vep.hip check_vep3: 3D VEP refuses blocks with (nx+2)(ny+2)(nz+2) >= 2^29"""
    nx, ny, nz = ni
    return (nx + 2) * (ny + 2) * (nz + 2) < 1 << 29


def batch2d(ni):
    """stokes2d.hip batch2: k_fused2d_b (u32 byte offsets) runs only when (nx+2)(ny+2) < 2^29"""
    nx, ny = ni
    return (nx + 2) * (ny + 2) < 1 << 29


def cells_fit_i32(ni):
    """(n+2)^3 < 2^31: element indices of every array fit a signed 32-bit int"""
    p = 1
    for n in ni:
        p *= n + 2
    return p < OFF31


# ---- staggered families -------------------------------------------------------------------------------------------------------------


def families(ni):
    """name -> extents of every staggered family of the Stokes arrays (arrays.py velocity_shapes / _tensor_shapes / residual_shapes)"""
    if len(ni) == 2:
        nx, ny = ni
        return {"cells": (nx, ny), "Vx": (nx + 1, ny + 2), "Vy": (nx + 2, ny + 1), "vertices": (nx + 1, ny + 1),
                "Rx": (nx - 1, ny), "Ry": (nx, ny - 1)}
    nx, ny, nz = ni
    return {"cells": (nx, ny, nz), "Vx": (nx + 1, ny + 2, nz + 2), "Vy": (nx + 2, ny + 1, nz + 2), "Vz": (nx + 2, ny + 2, nz + 1),
            "yz": (nx, ny + 1, nz + 1), "xz": (nx + 1, ny, nz + 1), "xy": (nx + 1, ny + 1, nz), "vertices": (nx + 1, ny + 1, nz + 1),
            "Rx": (nx - 1, ny, nz), "Ry": (nx, ny - 1, nz), "Rz": (nx, ny, nz - 1)}


def nbytes(ext):
    p = F64
    for n in ext:
        p *= n
    return p


def smallest_bytes(ni):
    return min(nbytes(e) for e in families(ni).values())


def largest_bytes(ni):
    return max(nbytes(e) for e in families(ni).values())


def cross_plane(ext):
    """index along the last axis of the plane (3D) / row (2D) that holds the first entry whose byte offset is >= 2^31 (None: the array stays below)"""
    if nbytes(ext) <= OFF31:
        return None
    plane = 1
    for n in ext[:-1]:
        plane *= n
    return (OFF31 // F64) // plane


def cross_planes(ni):
    """(first, last) crossing plane over the families that reach 2^31"""
    ks = [cross_plane(e) for e in families(ni).values()]
    ks = [k for k in ks if k is not None]
    return min(ks), max(ks)


# ---- device-memory budgets (counted from the code) -------------------------------------------------------------------------------------
# 3D StokesArrays (arrays.py): P, P0, ∇V, Q (4), V (3), U (3), τ and τ_o (9 each: 6 components + 3 centre copies of the shear stresses),
# ε (6; its centre copies are lazy), η (1), R (4) = 39; the test's K, G, ρg (3) = 5; the library's ητ (1); the handle's second state set (10)
STOKES3_ARRAYS = 39 + 5 + 1 + 10
# 2D: P, P0, ∇V, Q (4), V (2), U (2), τ and τ_o (4 each), ε (3), η (1), R (3) = 23; K, G, ρg (2) = 4; ητ (1); second state set (6)
STOKES2_ARRAYS = 23 + 4 + 1 + 6
# 3D VEP: the 65 arrays the driver takes (stokes.py vep_fields3d, all required), the single-phase ratios (centre, vertex, three edge families), ρg (3),
# and what the library holds for the driver (second sets of the state, ητ ping-pong, new normal stresses: 18 arrays, measured)
VEP3_ARRAYS = 65 + 5 + 3 + 18
KEEP3 = 21                  # device copies of the fused leg's results: P, τ (6), V (3), R (4), ∇V, ε (6)
KEEP2 = 6                   # P, τxx, τyy, τxy, Vx, Vy
BUDGET_BYTES = 200 * 10 ** 9
# the 3D VEP driver alone holds 91 arrays: no block whose smallest array is past 2 GiB fits 200 GB (HIGH3 has 1.5 % of cells to spare), so its tests
# get 220 GB of the 288 GB card
VEP3_BUDGET_BYTES = 220 * 10 ** 9


TEMPS = 2                   # transient arrays: the flat buffer of a random fill, the mask of a nonzero count
MARGIN = 8 * GiB            # allocator rounding, the driver's reduction and operand-check buffers, the small grids (measured peaks exceed the array count by 5 - 8 GB)


def budget(ni, narrays, keep=0):
    """bytes held at the peak of a test: every array counted at the size of the largest family, the transient arrays and a measured margin"""
    return (narrays + keep + TEMPS) * largest_bytes(ni) + MARGIN


def stokes3_budget():
    return budget(HIGH3, STOKES3_ARRAYS, KEEP3)


def stokes2_budget(ni):
    return budget(ni, STOKES2_ARRAYS, KEEP2)


def vep3_budget():
    return budget(HIGH3, VEP3_ARRAYS)          # the parity test keeps its comparison copies in host memory


# ---- the translated blob -------------------------------------------------------------------------------------------------------------
# One PT iteration reads, for a node, its neighbours one index away (stress from V, V from the stresses and P; the shear nodes average
# over one more index) and flow_bcs! copies across one face layer: a nonzero entry influences at most REACH indices per iteration, in every
# array and every direction.  SLACK covers the staggering between the families.
REACH = 2
SLACK = 2
BOX = 8
# the PT iterations of the GPU runs: iterations 1 .. ITER_MAX + 1; observed: the multiples of NOUT and the last; fused steps: 1, 2 and 5
ITER_MAX, NOUT = 6, 4
IT = ITER_MAX + 1


def radius(it):
    """how far (in indices, beyond the box) a blob can influence the state after `it` PT iterations"""
    return REACH * it + SLACK


def interior_box_start(ni):
    """first index of the interior box along each axis: centred in the leading axes, straddling the planes where the byte offsets of every
    family cross 2^31 along the last one"""
    k0, k1 = cross_planes(ni)
    lo = k0 - (BOX - (k1 - k0 + 1)) // 2
    return tuple(n // 2 - BOX // 2 for n in ni[:-1]) + (lo,)


def small_interior_start(small):
    return tuple(n // 2 - BOX // 2 for n in small)


def corner_region(ext, it):
    """slices (per axis, of an array of extents ext) of the region the high-corner box (the last BOX entries along every axis) can reach"""
    r = radius(it)
    return tuple(slice(max(e - BOX - r, 0), e) for e in ext)


def interior_region(start, ext, it):
    r = radius(it)
    return tuple(slice(max(s - r, 0), min(s + BOX + r, e)) for s, e in zip(start, ext))


def regions_clear(ni, it):
    """the two influence regions are disjoint, neither touches a low face, and the interior one keeps clear of every high face"""
    out = []
    st = interior_box_start(ni)
    for name, ext in families(ni).items():
        c = corner_region(ext, it)
        m = interior_region(st, ext, it)
        disjoint = any(a.stop <= b.start or b.stop <= a.start for a, b in zip(c, m))
        clear_lo = all(s.start > 0 for s in c) and all(s.start > 0 for s in m)
        clear_hi = all(s.stop < e for s, e in zip(m, ext))
        out.append((name, disjoint, clear_lo, clear_hi))
    return out


def small_regions_clear(small, it):
    """on the small grid: the corner region and the centred interior region each stay clear of the low faces (and the interior one of the high faces)"""
    out = []
    st = small_interior_start(small)
    for name, ext in families(small).items():
        c = corner_region(ext, it)
        m = interior_region(st, ext, it)
        out.append((name, all(s.start > 0 for s in c), all(s.start > 0 for s in m) and all(s.stop < e for s, e in zip(m, ext))))
    return out


def straddles(ni):
    """the interior box holds, along the last axis, every family's crossing plane with at least one plane below it and one above it"""
    st = interior_box_start(ni)[-1]
    k0, k1 = cross_planes(ni)
    return st < k0 and k1 < st + BOX - 1
