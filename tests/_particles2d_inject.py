"""NumPy restatement of operator 12 of include/jrx.h, inject_particles_phase! in gather form (k_pt_inject of csrc/particles.hip), operation for operation: the
same products and sums in the same order, each rounded once, the same scan orders and the same strict comparisons, so the device results are compared as bit
patterns.  Arrays are indexed as in tests/_particles2d.py: per-particle arrays [i, j, s], grid fields [i, j].
tests/test_particles2d_inject_restatement.py pins this text; tests/test_gpu_particles2d_inject.py holds the kernel to it."""
from __future__ import annotations

import numpy as np

import _particles2d as PT

COUNTS = ("n_active_before", "n_active_after", "n_deficient", "n_injected", "n_no_donor")
VERTEX, CENTRE, DONOR = 0, 1, 2


def _vertex_at(F, p, i, j, x, y):
    """operator 3's expression at (x, y) over the vertices of cell (i, j)"""
    xv, yv = p.x0 + float(i) * p.dx, p.y0 + float(j) * p.dy
    tx, ty = (x - xv) * p._dx, (y - yv) * p._dy
    return (1.0 - ty) * ((1.0 - tx) * F[i, j] + tx * F[i + 1, j]) + ty * ((1.0 - tx) * F[i, j + 1] + tx * F[i + 1, j + 1])


def _centre_at(F, p, x, y):
    """operator 6's interpolant at (x, y): (value, ok)"""
    v, ok = PT.interp(F, p.x0 + 0.5 * p.dx, p.y0 + 0.5 * p.dy, p._dx, p._dy, np.array([x]), np.array([y]))
    return float(v[0]), bool(ok[0])


def inject(p, pPhases, args=(), fields=(), field_loc=(), min_xcell=None, lattice=None):
    """(active_out, counts).  px, py of p, pPhases and every args[k] are written in place, and only in slots inactive at entry; p.active is not written: the
    caller makes active_out the mask.  lattice = (nsx, nsy), by default that of p.nxcell."""
    nx, ny, mx = p.nx, p.ny, p.max_xcell
    min_xcell = p.min_xcell if min_xcell is None else int(min_xcell)
    nsx, nsy = PT.lattice(p.nxcell) if lattice is None else lattice
    assert len(args) == len(fields) == len(field_loc) and 1 <= min_xcell <= mx and min_xcell <= nsx * nsy <= 64
    assert all(loc in (VERTEX, CENTRE, DONOR) for loc in field_loc) and (CENTRE not in field_loc or (nx >= 2 and ny >= 2))
    hx, hy = p.dx / nsx, p.dy / nsy
    act = p.active
    out = act.copy()
    c = dict.fromkeys(COUNTS, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(ny):
            for i in range(nx):
                n = int((act[i, j] != 0).sum())
                c["n_active_before"] += n
                if n >= min_xcell:
                    c["n_active_after"] += n
                    continue
                c["n_deficient"] += 1
                xc, yc = p.x0 + float(i) * p.dx, p.y0 + float(j) * p.dy
                occ = set()
                for s in range(mx):
                    if not act[i, j, s]:
                        continue
                    a = np.floor(((p.px[i, j, s] - xc) * p._dx) * float(nsx))
                    b = np.floor(((p.py[i, j, s] - yc) * p._dy) * float(nsy))
                    if a >= 0.0 and a < float(nsx) and b >= 0.0 and b < float(nsy):
                        occ.add(int(a) + nsx * int(b))
                free = 0
                for q in range(nsx * nsy):
                    if not n < min_xcell:
                        break
                    if q in occ:
                        continue
                    a, b = q % nsx, q // nsx
                    x, y = xc + (float(a) + 0.5) * hx, yc + (float(b) + 0.5) * hy
                    best, donor = np.inf, None
                    cells = [(i, j)] + [(i + di, j + dj) for dj in (-1, 0, 1) for di in (-1, 0, 1) if (di, dj) != (0, 0)]
                    for ic, jc in cells:
                        if not (0 <= ic < nx and 0 <= jc < ny):
                            continue
                        for s in range(mx):
                            if not act[ic, jc, s]:
                                continue
                            ex, ey = p.px[ic, jc, s] - x, p.py[ic, jc, s] - y
                            d2 = ex * ex + ey * ey
                            if d2 < best:
                                best, donor = d2, (ic, jc, s)
                    if donor is None:
                        c["n_no_donor"] += 1
                        break
                    while act[i, j, free]:
                        free += 1
                    to = (i, j, free)
                    free += 1
                    p.px[to], p.py[to], out[to] = x, y, 1
                    pPhases[to] = pPhases[donor]
                    for A, F, loc in zip(args, fields, field_loc):
                        if loc == DONOR:
                            A[to] = A[donor]
                        elif loc == VERTEX:
                            A[to] = _vertex_at(F, p, i, j, x, y)
                        else:
                            v, ok = _centre_at(F, p, x, y)
                            if ok:
                                A[to] = v
                    n += 1
                    c["n_injected"] += 1
                c["n_active_after"] += n
    return out, c
