"""NumPy restatement of operators 6 - 9 of the section "2D marker-in-cell particles" of include/jrx.h -- centroid2particle!, particle2centroid!,
rotate_stress_particles!, and the two calls of a time step, rotate_stress!(pτxx, pτyy, pτxy, pω, stokes, particles, dt) and stress2grid! -- operation for
operation with csrc/particles.hip: the same products and sums in the same order, each rounded once.  The interpolant, the weights and the vertex operators come
from tests/_particles2d.py, the per-point rotation from tests/_stress_rotation.py.  Per-particle arrays are indexed [i, j, s]; grid fields [i, j].
tests/test_particles2d_stress_restatement.py pins this text; tests/test_gpu_particles2d_stress.py holds the kernels to it."""
from __future__ import annotations

import numpy as np

from _particles2d import _w, grid2particle, interp, particle2grid
from _stress_rotation import rot2

TAU_O = ("xx", "yy", "xy_c", "xy", "xx_v", "yy_v")          # the member order of jrx_rotate_stress2d


# ---------------------------------------------------------------------------------------------- 6. centroid2particle
def centroid2particle(pF, F, p):
    """the new pF: A(x, y) per active slot, 0 in an inactive one, pF itself where a scaled coordinate is not finite"""
    assert F.shape == (p.nx, p.ny) and p.nx >= 2 and p.ny >= 2
    ox, oy = p.x0 + 0.5 * p.dx, p.y0 + 0.5 * p.dy
    v, ok = interp(F, ox, oy, p._dx, p._dy, p.px, p.py)
    return np.where(p.active != 0, np.where(ok, v, pF), 0.0)


# ---------------------------------------------------------------------------------------------- 7. particle2centroid
def centroid_sums(pF, p, i, j):
    """(num, den) of cell (i, j): its own bucket in slot order"""
    xc, yc = p.x0 + (float(i) + 0.5) * p.dx, p.y0 + (float(j) + 0.5) * p.dy
    num = den = 0.0
    for s in range(p.max_xcell):
        if not p.active[i, j, s]:
            continue
        w = _w(p.px[i, j, s], xc, p._dx) * _w(p.py[i, j, s], yc, p._dy)
        num = num + w * pF[i, j, s]
        den = den + w
    return num, den


def particle2centroid(F, pF, p):
    """returns the new F (F itself where no weight arrives)"""
    assert F.shape == (p.nx, p.ny)
    out = F.copy()
    for i in range(p.nx):
        for j in range(p.ny):
            num, den = centroid_sums(pF, p, i, j)
            if not den == 0.0:
                out[i, j] = num / den
    return out


def centre_den(p):
    one = np.ones(p.px.shape)
    return np.array([[centroid_sums(one, p, i, j)[1] for j in range(p.ny)] for i in range(p.nx)])


def vertex_den(p):
    """the denominators of particle2grid: num of the constant 1 is den"""
    den = np.zeros((p.nx + 1, p.ny + 1))
    for i in range(p.nx + 1):
        xv = p.x0 + float(i) * p.dx
        for j in range(p.ny + 1):
            yv = p.y0 + float(j) * p.dy
            d = 0.0
            for oi in (-1, 0):
                for oj in (-1, 0):
                    ic, jc = i + oi, j + oj
                    if not (0 <= ic < p.nx and 0 <= jc < p.ny):
                        continue
                    for s in range(p.max_xcell):
                        if p.active[ic, jc, s]:
                            d = d + _w(p.px[ic, jc, s], xv, p._dx) * _w(p.py[ic, jc, s], yv, p._dy)
            den[i, j] = d
    return den


# ---------------------------------------------------------------------------------------------- 8. rotation on the particles
def rotate(pτ, pω, p, dt, method="matrix"):
    """the new (pτxx, pτyy, pτxy): rotated by θ = dt pω per active slot, untouched elsewhere"""
    xx, yy, xy = pτ
    with np.errstate(invalid="ignore", over="ignore"):
        oxx, oyy, oxy = rot2(xx, yy, xy, dt * pω, method)
    a = p.active != 0
    return np.where(a, oxx, xx), np.where(a, oyy, yy), np.where(a, oxy, xy)


# ---------------------------------------------------------------------------------------------- 9. the two calls of a time step
def rotate_stress(pτ, pω, τxx, τyy, τxy, ωxy, p, dt, method="matrix"):
    """the new (pτxx, pτyy, pτxy, pω): operator 6 for xx and yy, operator 3 for xy and ω, then operator 8.  pω is an argument only because the chain overwrites
    it in full: its old contents do not matter"""
    xx, yy = centroid2particle(pτ[0], τxx, p), centroid2particle(pτ[1], τyy, p)
    xy, w = grid2particle(τxy, p), grid2particle(ωxy, p)
    return rotate((xx, yy, xy), w, p, dt, method) + (w,)


def stress2grid(τ_o, pτ, p):
    """the new τ_o as a dict over TAU_O: xx, yy, xy_c by operator 7, xx_v, yy_v, xy by operator 4"""
    pxx, pyy, pxy = pτ
    return dict(xx=particle2centroid(τ_o["xx"], pxx, p), yy=particle2centroid(τ_o["yy"], pyy, p), xy_c=particle2centroid(τ_o["xy_c"], pxy, p),
                xy=particle2grid(τ_o["xy"], pxy, p), xx_v=particle2grid(τ_o["xx_v"], pxx, p), yy_v=particle2grid(τ_o["yy_v"], pyy, p))
