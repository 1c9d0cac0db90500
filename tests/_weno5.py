"""NumPy restatement of the reference's WENO-5 advection (src/advection/weno5.jl), written from its formulas; the checker of the tests of
WENO_advection_.  Arrays are (nx, ny) with x first, as in Julia.  No fma here (NumPy has none), so the device results agree to rounding, not bit for bit.

  constants            src/types/constructors/weno.jl:7-24
  betas                weno5.jl:10-16    β0 = c1 (u1 - 2u2 + u3)² + c2 (u1 - 4u2 + 3u3)², β1, β2 likewise
  alphas               weno5.jl:23-55    JS (method 1): d / (β + ϵ)²;  Z (method 2): d (1 + (τ / (β + ϵ))²), τ = |β0 - β2|
  candidates           weno5.jl:59-71    upwind s0 = sc1 u1 - sc2 u2 + sc3 u3, ...; downwind s0 = -sc4 u1 + sc5 u2 + sc1 u3, ...
  weights, flux        weno5.jl:84-107   w = α / Σα, f = Σ w s
  clamped stencils     weno5.jl:120-151  fB / fT along x from u[i-2..i+2, j], fL / fR along y from u[i, j-2..j+2], indices clamped to the box of u
  weno_rhs             weno5.jl:154-168  r = max(vx,0)(fB[i]-fB[iS])/dx + min(vx,0)(fT[iN]-fT[i])/dx + max(vy,0)(fL[j]-fL[jW])/dy + min(vy,0)(fR[jE]-fR[j])/dy
  SSP-RK3              weno5.jl:195-230  u1 = u - dt r(u); ut = 3/4 u + 1/4 u1 - 1/4 dt r(u1); u = 1/3 u + 2/3 ut - 2/3 dt r(ut)
"""
import numpy as np

D_UP = (1 / 10, 3 / 5, 3 / 10)
D_DN = (3 / 10, 3 / 5, 1 / 10)
C1, C2 = 13 / 12, 1 / 4
SC1, SC2, SC3, SC4, SC5 = 1 / 3, 7 / 6, 11 / 6, 1 / 6, 5 / 6
EPS = 1.0e-6


def _flux(u1, u2, u3, u4, u5, method, upwind):
    b = (C1 * (u1 - 2 * u2 + u3) ** 2 + C2 * (u1 - 4 * u2 + 3 * u3) ** 2,
         C1 * (u2 - 2 * u3 + u4) ** 2 + C2 * (u2 - u4) ** 2,
         C1 * (u3 - 2 * u4 + u5) ** 2 + C2 * (3 * u3 - 4 * u4 + u5) ** 2)
    d = D_UP if upwind else D_DN
    if method == 1:
        a = [d[k] * (1 / (b[k] + EPS)) ** 2 for k in range(3)]
    elif method == 2:
        tau = np.abs(b[0] - b[2])
        a = [d[k] * (1 + (tau * (1 / (b[k] + EPS))) ** 2) for k in range(3)]
    else:
        raise ValueError("Unknown method for the WENO Scheme")
    s = 1 / (a[0] + a[1] + a[2])
    w = [x * s for x in a]
    if upwind:
        c = (SC1 * u1 - SC2 * u2 + SC3 * u3, -SC4 * u2 + SC5 * u3 + SC1 * u4, SC1 * u3 + SC5 * u4 - SC4 * u5)
    else:
        c = (-SC4 * u1 + SC5 * u2 + SC1 * u3, SC1 * u2 + SC5 * u3 - SC4 * u4, SC3 * u3 - SC2 * u4 + SC1 * u5)
    return w[0] * c[0] + w[1] * c[1] + w[2] * c[2]


def fluxes(u, method):
    """weno_f!(u): (fL, fR, fB, fT) over the box of u"""
    nx, ny = u.shape
    ii, jj = np.arange(nx), np.arange(ny)
    sx = [u[np.clip(ii + o, 0, nx - 1), :] for o in (-2, -1, 0, 1, 2)]
    sy = [u[:, np.clip(jj + o, 0, ny - 1)] for o in (-2, -1, 0, 1, 2)]
    return _flux(*sy, method, True), _flux(*sy, method, False), _flux(*sx, method, True), _flux(*sx, method, False)


def rhs(u, vx, vy, dx, dy, method):
    """weno_rhs over the box of u; vx, vy are read at [i, j] of their own (possibly larger) extents"""
    nx, ny = u.shape
    fL, fR, fB, fT = fluxes(u, method)
    vx, vy = vx[:nx, :ny], vy[:nx, :ny]
    iS, iN = np.clip(np.arange(nx) - 1, 0, nx - 1), np.clip(np.arange(nx) + 1, 0, nx - 1)
    jW, jE = np.clip(np.arange(ny) - 1, 0, ny - 1), np.clip(np.arange(ny) + 1, 0, ny - 1)
    _dx, _dy = 1 / dx, 1 / dy
    return (np.maximum(vx, 0) * (fB - fB[iS, :]) * _dx + np.minimum(vx, 0) * (fT[iN, :] - fT) * _dx
            + np.maximum(vy, 0) * (fL - fL[:, jW]) * _dy + np.minimum(vy, 0) * (fR[:, jE] - fR) * _dy)


def advect(u, vx, vy, dx, dy, dt, method):
    """WENO_advection!: returns (u after the call, weno.ut = the stage-2 field, (fL, fR, fB, fT) of the stage-2 field -- what the reference's six-launch
    form leaves in the flux arrays)"""
    u = np.asarray(u, dtype=np.float64)
    u1 = u - dt * rhs(u, vx, vy, dx, dy, method)
    ut = 0.75 * u + 0.25 * u1 - 0.25 * dt * rhs(u1, vx, vy, dx, dy, method)
    one_third = 1 / 3
    two_thirds = 2 * one_third
    f = fluxes(ut, method)
    unew = one_third * u + two_thirds * ut - two_thirds * dt * rhs(ut, vx, vy, dx, dy, method)
    return unew, ut, f


def gaussian_case(n, method, *, run=None):
    """the accuracy case: exp(-|x - (0.35, 0.4)|² / 0.01) on the unit square with n + 1 vertices per direction, v = (1, 0.5), CFL 0.4, T = 0.2.
    run(u, vx, vy, dx, dt, nt) advances nt steps (default: the restatement).  Returns (u at T, exact solution, L1 error)."""
    x = np.linspace(0.0, 1.0, n + 1)
    X, Y = np.meshgrid(x, x, indexing="ij")
    dx = 1.0 / n

    def g(X, Y):
        return np.exp(-((X - 0.35) ** 2 + (Y - 0.4) ** 2) / 0.01)

    u = g(X, Y)
    vx, vy = np.full_like(u, 1.0), np.full_like(u, 0.5)
    T = 0.2
    nt = int(round(T / (0.4 * dx)))
    dt = T / nt
    if run is None:
        for _ in range(nt):
            u = advect(u, vx, vy, dx, dx, dt, method)[0]
    else:
        u = run(u, vx, vy, dx, dt, nt)
    exact = g(X - T, Y - 0.5 * T)
    return u, exact, float(np.abs(u - exact).mean())


def sample_field(nx, ny, rng):
    """a smooth field plus a step plus a constant patch (drives the weights away from the linear ones and puts β at 0)"""
    x = np.linspace(0, 1, nx)[:, None]
    y = np.linspace(0, 1, ny)[None, :]
    u = 1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(3 * np.pi * y) + 0.05 * rng.standard_normal((nx, ny))
    u = u + np.where(x + 0.3 * y > 0.55, 0.8, 0.0)
    u[: max(1, nx // 4), : max(1, ny // 4)] = 2.5
    return u
