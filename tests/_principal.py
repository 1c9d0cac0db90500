"""NumPy restatement of the reference's principal-stress kernels (src/stokes/PrincipalStresses.jl), written from its formulas; the checker of the tests of
compute_principal_stresses_.  Arrays are (ndim, ni...) with the component first, as in Julia.

  2D  PrincipalStresses.jl:14-40   a = (xx + yy)/2, b = √((xx − yy)²/2 + xy²), θ = atan(2xy / (xx − yy))/2, σ1 = (a + b)(cosθ, sinθ), σ2 = (a − b)(−sinθ, cosθ)
  3D  PrincipalStresses.jl:42-141  Householder to Hessenberg form, then at most 50 QR steps shifted by H[3,3], stopped when every off-diagonal |H_ij| < 1e-10;
                                   σ = diag(H) sorted by reverse(sortperm), σ_j = σ[j] · (Q_hess V)[:, perm_j].  The signs of the vectors follow the QR
                                   factorisation used (StaticArrays' there, LAPACK's here), so only the eigenvalues and |vectors| are comparable.
"""
import numpy as np


def principal2d(xx, yy, xy):
    """(σ1, σ2), each (2, ni...), for the cell-centred components xx, yy, xy_c"""
    with np.errstate(all="ignore"):
        a = (xx + yy) / 2
        d = xx - yy
        b = np.sqrt(d * d / 2 + xy * xy)
        th = np.arctan(2 * xy / d) / 2
        sn, cs = np.sin(th), np.cos(th)
        l1, l2 = a + b, a - b
        return np.stack([l1 * cs, l1 * sn]), np.stack([l2 * -sn, l2 * cs])


def _hessenberg_3x3(A):
    """PrincipalStresses.jl:111-141"""
    x = A[1:, 0]
    alpha = np.linalg.norm(x)
    if alpha == 0:
        Qs = np.eye(2)
    else:
        v = x + np.sign(x[0]) * alpha * np.array([1.0, 0.0])
        v = v / np.linalg.norm(v)
        Qs = np.eye(2) - 2 * np.outer(v, v)
    Q = np.eye(3)
    Q[1:, 1:] = Qs
    return (Q.T @ A) @ Q, Q


def hessenberg_eigen_3x3(A, tol=1.0e-10, max_iter=50):
    """PrincipalStresses.jl:67-97: (σ_1, σ_2, σ_3 vectors, converged, iterations)"""
    H, Qh = _hessenberg_3x3(np.asarray(A, dtype=np.float64))
    V = np.eye(3)
    converged, it = False, 0
    for it in range(1, max_iter + 1):
        lam = H[2, 2] * np.eye(3)
        Q, R = np.linalg.qr(H - lam)
        H = R @ Q + lam
        V = V @ Q
        off = np.abs(H[~np.eye(3, dtype=bool)])
        if np.all(off < tol):
            converged = True
            break
    e = Qh @ V
    s = np.diag(H)
    perms = np.argsort(s, kind="stable")[::-1]
    s = s[perms]
    return tuple(s[j] * e[:, perms[j]] for j in range(3)), converged, it


def tensor3(xx, yy, zz, yz, xz, xy):
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=np.float64)


# test/test_types.jl:222-238: the reference's own 3D case and what it asserts (Σ |σ_j| = 6 within 1e-6)
REFERENCE_CASE = dict(xx=1.0, yy=2.0, zz=3.0, xy=0.5, xz=0.25, yz=0.75)
REFERENCE_EIGENVALUES = (3.48702452, 1.721857, 0.79111848)       # to the digits quoted for it


def sign_normalised(e):
    """unit vector e with its largest-magnitude component positive (the lowest index on ties) -- the device's convention"""
    k = int(np.argmax(np.abs(e)))
    return -e if e[k] < 0 else e
