"""NumPy restatement of the 3D form of the WENO-5 advection (jrx_weno5_advection3d): tests/_weno5.py one dimension up.  The reference defines the scheme one
direction at a time (src/advection/weno5.jl:10-168), so the 3D form is determined: the same clamped five-point reconstruction along z, two more terms in
weno_rhs, the same SSP-RK3.  Arrays are (nx, ny, nz) with x first, as in Julia.  No fma here, so the device results agree to rounding, not bit for bit.

  fluxes    fB / fT along x from u[i-2..i+2, j, k], fL / fR along y from u[i, j-2..j+2, k], fD / fU along z from u[i, j, k-2..k+2] (upwind / downwind; fD, fU
            are this project's names), indices clamped to the box of u
  weno_rhs  the four terms of weno5.jl:154-168, then max(vz,0)(fD[k]-fD[kD])/dz + min(vz,0)(fU[kU]-fU[k])/dz, summed left to right
"""
import numpy as np

from _weno5 import _flux, sample_field  # noqa: F401  (sample_field: for the tests that build 3D fields from 2D ones)


def fluxes3(u, method):
    """(fL, fR, fB, fT, fD, fU) over the box of u"""
    out = {}
    for ax in range(3):
        n = u.shape[ax]
        idx = np.arange(n)
        s = [np.take(u, np.clip(idx + o, 0, n - 1), axis=ax) for o in (-2, -1, 0, 1, 2)]
        out[ax] = (_flux(*s, method, True), _flux(*s, method, False))
    return out[1][0], out[1][1], out[0][0], out[0][1], out[2][0], out[2][1]


def _shift(f, ax, o):
    n = f.shape[ax]
    return np.take(f, np.clip(np.arange(n) + o, 0, n - 1), axis=ax)


def rhs3(u, vx, vy, vz, dx, dy, dz, method):
    """weno_rhs over the box of u; the velocities are read at [i, j, k] of their own (possibly larger) extents"""
    nx, ny, nz = u.shape
    fL, fR, fB, fT, fD, fU = fluxes3(u, method)
    vx, vy, vz = (v[:nx, :ny, :nz] for v in (vx, vy, vz))
    _dx, _dy, _dz = 1 / dx, 1 / dy, 1 / dz
    return (np.maximum(vx, 0) * (fB - _shift(fB, 0, -1)) * _dx + np.minimum(vx, 0) * (_shift(fT, 0, 1) - fT) * _dx
            + np.maximum(vy, 0) * (fL - _shift(fL, 1, -1)) * _dy + np.minimum(vy, 0) * (_shift(fR, 1, 1) - fR) * _dy
            + np.maximum(vz, 0) * (fD - _shift(fD, 2, -1)) * _dz + np.minimum(vz, 0) * (_shift(fU, 2, 1) - fU) * _dz)


def advect3(u, vx, vy, vz, dx, dy, dz, dt, method):
    """returns (u after the call, weno.ut = the stage-2 field, (fL, fR, fB, fT, fD, fU) of the stage-2 field -- what the six-launch form leaves)"""
    u = np.asarray(u, dtype=np.float64)
    u1 = u - dt * rhs3(u, vx, vy, vz, dx, dy, dz, method)
    ut = 0.75 * u + 0.25 * u1 - 0.25 * dt * rhs3(u1, vx, vy, vz, dx, dy, dz, method)
    one_third = 1 / 3
    two_thirds = 2 * one_third
    f = fluxes3(ut, method)
    unew = one_third * u + two_thirds * ut - two_thirds * dt * rhs3(ut, vx, vy, vz, dx, dy, dz, method)
    return unew, ut, f


def gaussian_case3(n, method, *, run=None):
    """the accuracy case: exp(-|x - (0.35, 0.4, 0.45)|² / 0.01) on the unit cube with n + 1 vertices per direction, v = (1, 0.5, -0.25), CFL 0.4, T = 0.2.
    run(u, vx, vy, vz, dx, dt, nt) advances nt steps (default: the restatement).  Returns (u at T, exact solution, L1 error)."""
    x = np.linspace(0.0, 1.0, n + 1)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    dx = 1.0 / n

    def g(X, Y, Z):
        return np.exp(-((X - 0.35) ** 2 + (Y - 0.4) ** 2 + (Z - 0.45) ** 2) / 0.01)

    u = g(X, Y, Z)
    vx, vy, vz = np.full_like(u, 1.0), np.full_like(u, 0.5), np.full_like(u, -0.25)
    T = 0.2
    nt = int(round(T / (0.4 * dx)))
    dt = T / nt
    if run is None:
        for _ in range(nt):
            u = advect3(u, vx, vy, vz, dx, dx, dx, dt, method)[0]
    else:
        u = run(u, vx, vy, vz, dx, dt, nt)
    exact = g(X - T, Y - 0.5 * T, Z + 0.25 * T)
    return u, exact, float(np.abs(u - exact).mean())
