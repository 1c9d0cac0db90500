"""NumPy restatement of the reference's pseudo-transient heat diffusion, written from its formulas, 2D and 3D, in a chosen precision (np.float64 or
np.longdouble); the checker of tests/test_heat_diffusion_restatement.py (the CPU oracle) and tests/test_gpu_heat_diffusion_inputs.py (the device), and the
builder of their inputs.  Arrays are (nx, ny[, nz]) with x first, as in Julia; T, Told, ΔT carry one ghost layer.  Whole-array expressions, no fma.

  compute_flux!   src/thermal_diffusion/DiffusionPT_kernels.jl:6-61 (3D), :327-364 (2D)   on face f of an axis with n cells: l = clamp(f - 1), r = clamp(f) (to 1..n),
                  K = (K[l] + K[r]) / 2, θ = (θr_dτ[l] + θr_dτ[r]) / 2, q2 = -K (T[f + 1] - T[f]) _d, q = (q θ + q2) / (1 + θ); a constant_flux face writes q = value
                  and leaves q2 as it was.  Rheology form (:63-158, :366-440 as the project evaluates it): K = (k + k) / 2 with a constant k
  update_T!       :160-199, :519-551      T = (dτ_ρ (-(Σ_d (q[+1] - q) _d) + Told ρCp _dt + H + shear_heating) + T) / (1 + dτ_ρ ρCp _dt) on the interior
                  rheology form (:201-248, :553-601): ρCp = Cp (ρ0 (1 - α (T - T0))) from the cell's T before the update; no adiabatic term here
  check_res!      :250-282, :603-629      ResT = -ρCp (T - Told) _dt - Σ_d (q2[+1] - q2) _d + H + shear_heating
  update_ΔT!      :670-673                ΔT = T - Told, ghosts included
  thermal_bcs!    src/boundaryconditions/BoundaryConditions.jl:46-54: constant_value, then no_flux, then periodic, each one kernel whose statements are, in this order,
                  2D (constant_value.jl:1-13, free_slip.jl:72-84, periodic.jl:1-13): bot, top over every i (ghost columns included), then left, right over every j;
                  3D (constant_value.jl:15-33, free_slip.jl:86-103, periodic.jl:37-54): bot, top (k = 1, end), then left, right, then front, back (j = 1, end).
                  constant_value: ghost = 2 value - inner; no_flux: ghost = inner; periodic: ghost = the inner layer of the opposite face.
                  Here every statement runs over its whole face before the next one starts: a later statement sees what an earlier one wrote on the ghost edges and
                  corners, which is the order the project's oracle and BC kernels keep.
  PT loop         src/thermal_diffusion/DiffusionPT_solver.jl:34-149 (:181-305 rheology form): Told = T; while err > ϵ and iter < iterMax: compute_flux!, update_T!,
                  thermal_bcs!; iter += 1; every nout: check_res!, err = norm(ResT) / sqrt(length(ResT)), recorded with iter; at the end update_ΔT!
  PTThermalCoeffs src/thermal_diffusion/DiffusionPT_coefficients.jl:17-26   (taken from the project's own evaluation: an input of the loop here, not restated)

  optional terms  f["adiabatic"] (rheology form only, :553-601, :631-668): + adiabatic T inside the bracket of update_T! (T before the update) and in check_res!;
                  f["dirichlet_mask"] (the shape of T; with f["dirichlet_value"], an array, or f["dirichlet_const"], a 0-d array): a cell whose mask is not zero takes
                  (1 - m) T + m value (apply_mask!, src/mask/mask.jl:49-50) instead of the update and has ResT = 0 (isNotDirichlet, :1-2, :619)
  N > 1           heatdiffusion_PT_blocks: the same loop on the blocks of an ImplicitGlobalGrid decomposition, update_halo!(thermal.T) after thermal_bcs! (:110)

Not restated: the phase-ratio form, non-uniform spacing.

The field names are those of the oracle's dictionaries: T, Told, dT, qTx, qTy[, qTz], qTx2, ..., H, shear_heating, ResT, K, rhoCp, thetar_dtau, dtau_rho.
"""
from types import SimpleNamespace

import numpy as np

FACES = {2: ("left", "right", "top", "bot"), 3: ("left", "right", "front", "back", "top", "bot")}
# face -> (axis, high side); 2D: bot / top are j = 1 / end; 3D: front / back are j = 1 / end, bot / top k = 1 / end
AXIS = {2: dict(left=(0, 0), right=(0, 1), bot=(1, 0), top=(1, 1)),
        3: dict(left=(0, 0), right=(0, 1), front=(1, 0), back=(1, 1), bot=(2, 0), top=(2, 1))}
BC_ORDER = {2: (("bot", "top"), ("left", "right")), 3: (("bot", "top"), ("left", "right"), ("front", "back"))}
QNAMES = ("qTx", "qTy", "qTz")


def _at(nd, ax, i):
    idx = [slice(None)] * nd
    idx[ax] = i
    return tuple(idx)


def _is_value(v):
    """`bc.left === false ? ... : 2 * bc.left - T`: anything but false is a value (true counts as 1)"""
    return v is not False and v is not None


def _is_flux(v):
    """`!isa(bc_flux.left, Bool)`"""
    return not isinstance(v, bool) and v is not None


def thermal_bcs(T, bc):
    nd = T.ndim
    for kind in ("constant_value", "no_flux", "periodic"):
        d = getattr(bc, kind)
        for pair in BC_ORDER[nd]:
            ax = AXIS[nd][pair[0]][0]
            for face, ghost, inner, opposite in ((pair[0], 0, 1, -2), (pair[1], -1, -2, 1)):
                v = d.get(face, False)
                if kind == "constant_value":
                    if _is_value(v):
                        T[_at(nd, ax, ghost)] = 2 * T.dtype.type(v) - T[_at(nd, ax, inner)]
                elif v:
                    T[_at(nd, ax, ghost)] = T[_at(nd, ax, inner if kind == "no_flux" else opposite)]


def compute_flux(f, _di, bc, rheology=None):
    T, th = f["T"], f["thetar_dtau"]
    nd, dt = T.ndim, T.dtype.type
    inner = [slice(1, -1)] * nd
    for ax in range(nd):
        n = th.shape[ax]
        face = np.arange(n + 1)
        l, r = np.clip(face - 1, 0, n - 1), np.clip(face, 0, n - 1)
        if rheology is None:
            K = (np.take(f["K"], l, axis=ax) + np.take(f["K"], r, axis=ax)) * dt(0.5)
        else:
            K = (dt(rheology["k"]) + dt(rheology["k"])) * dt(0.5)
        θ = (np.take(th, l, axis=ax) + np.take(th, r, axis=ax)) * dt(0.5)
        hi, lo = list(inner), list(inner)
        hi[ax], lo[ax] = slice(1, None), slice(0, -1)
        q, q2 = f[QNAMES[ax]], f[QNAMES[ax] + "2"]
        qv = -K * (T[tuple(hi)] - T[tuple(lo)]) * dt(_di[ax])
        qn = (q * θ + qv) / (dt(1) + θ)
        for name, (a, side) in AXIS[nd].items():
            v = bc.constant_flux.get(name, False)
            if a == ax and _is_flux(v):
                at = _at(nd, ax, -1 if side else 0)
                qn[at] = dt(v)
                qv[at] = q2[at]
        q[...] = qn
        q2[...] = qv


def _rhoCp(f, rheology):
    if rheology is None:
        return f["rhoCp"]
    dt = f["T"].dtype.type
    Tc = f["T"][(slice(1, -1),) * f["T"].ndim]
    return dt(rheology["Cp"]) * (dt(rheology["rho0"]) * (dt(1) - dt(rheology["alpha"]) * (Tc - dt(rheology.get("T0", 0.0)))))


def _div(f, _di, suffix):
    nd, dt = f["T"].ndim, f["T"].dtype.type
    out = None
    for ax in range(nd):
        q = f[QNAMES[ax] + suffix]
        term = (q[_at(nd, ax, slice(1, None))] - q[_at(nd, ax, slice(0, -1))]) * dt(_di[ax])
        out = term if out is None else out + term
    return out


def _adiabatic(f, rheology):
    """thermal.adiabatic enters the rheology forms only"""
    return f.get("adiabatic") if rheology is not None else None


def _dirichlet(f):
    """(mask on the cells, value on the cells) or (None, None)"""
    m = f.get("dirichlet_mask")
    if m is None:
        return None, None
    inner = (slice(1, -1),) * m.ndim
    v = f["dirichlet_value"][inner] if f.get("dirichlet_value") is not None else m.dtype.type(f["dirichlet_const"])
    return m[inner], v


def update_T(f, _di, _dt, rheology=None):
    T = f["T"]
    inner = (slice(1, -1),) * T.ndim
    one = T.dtype.type(1)
    ρCp, dτ_ρ, Tc = _rhoCp(f, rheology), f["dtau_rho"], T[inner].copy()
    src = -_div(f, _di, "") + f["Told"][inner] * ρCp * _dt + f["H"] + f["shear_heating"]
    if _adiabatic(f, rheology) is not None:
        src = src + f["adiabatic"] * Tc
    Tn = (dτ_ρ * src + Tc) / (one + dτ_ρ * ρCp * _dt)
    m, v = _dirichlet(f)
    if m is not None:
        Tn = np.where(m != 0, (one - m) * Tc + m * v, Tn)
    T[inner] = Tn


def check_res(f, _di, _dt, rheology=None):
    inner = (slice(1, -1),) * f["T"].ndim
    res = -_rhoCp(f, rheology) * (f["T"][inner] - f["Told"][inner]) * _dt - _div(f, _di, "2") + f["H"] + f["shear_heating"]
    if _adiabatic(f, rheology) is not None:
        res = res + f["adiabatic"] * f["T"][inner]
    m, _ = _dirichlet(f)
    if m is not None:
        res = np.where(m != 0, f["T"].dtype.type(0), res)
    f["ResT"][...] = res


def res_term_scale(f, _di, dt, rheology=None):
    """largest magnitude among the terms check_res! adds up: the scale its rounding lives on where the residual itself has cancelled"""
    inner = (slice(1, -1),) * f["T"].ndim
    _dt = 1 / f["T"].dtype.type(dt)
    terms = (_rhoCp(f, rheology) * (f["T"][inner] - f["Told"][inner]) * _dt, _div(f, _di, "2"), f["H"], f["shear_heating"])
    if _adiabatic(f, rheology) is not None:
        terms += (f["adiabatic"] * f["T"][inner],)
    return float(max(np.abs(t).max() for t in terms))


def heatdiffusion_PT(f, bc, _di, dt, *, iterMax, nout, eps=0.0, rheology=None):
    """the PT loop on the dictionary f (arrays of one dtype, changed in place); returns dict(iter_count, norm_ResT)"""
    T = f["T"]
    dtype = T.dtype.type
    _dt = 1 / dtype(dt)
    _sq = 1 / np.sqrt(dtype(f["ResT"].size))
    f["Told"][...] = T
    it, err, iter_count, norm_ResT = 0, 2 * eps if eps > 0 else np.inf, [], []
    while err > eps and it < iterMax:
        compute_flux(f, _di, bc, rheology)
        update_T(f, _di, _dt, rheology)
        thermal_bcs(T, bc)
        it += 1
        if it % nout == 0:
            check_res(f, _di, _dt, rheology)
            err = np.sqrt((f["ResT"] * f["ResT"]).sum()) * _sq
            norm_ResT.append(err)
            iter_count.append(it)
    f["dT"][...] = T - f["Told"]
    return dict(iter_count=np.array(iter_count, dtype=np.int64), norm_ResT=np.array(norm_ResT, dtype=T.dtype))


def heatdiffusion_PT_blocks(fs, bc, _di, dt, n, carts, L, *, iterMax, nout, eps=0.0, rheology=None, stop="max"):
    """the PT loop on the blocks fs[r] (one dictionary per rank, every rank with the same bc: the reference applies thermal_bcs! and the constant-flux faces on every
    face of the local array, and update_halo!(thermal.T) then replaces the ghost planes that have a neighbour, DiffusionPT_solver.jl:104-111).  n: cells of a
    local block, carts: jrx_cart of every rank, L: the library (jrx_halo_planes names the planes; a rank that is its own periodic neighbour copies from itself).
    stop = "local": every rank tests its own norm, as the reference does (:131, no reduction) -- a rank that has left neither computes nor receives any more,
    the others go on with the planes it left behind (an MPI run would wait for it for ever); stop = "max": every rank tests the maximum of the local norms,
    so all leave together, and still records its own.  Returns one dict(iter_count, norm_ResT, iterations) per rank."""
    import _blocks
    nr = len(fs)
    dtype = fs[0]["T"].dtype.type
    _dt = 1 / dtype(dt)
    _sq = 1 / np.sqrt(dtype(fs[0]["ResT"].size))
    for f in fs:
        f["Told"][...] = f["T"]
    err = [2 * eps if eps > 0 else np.inf] * nr          # what each rank's loop test sees
    it, done = 0, [0] * nr
    iter_count, norm_ResT = [[] for _ in range(nr)], [[] for _ in range(nr)]
    while it < iterMax and any(e > eps for e in err):
        active = [e > eps for e in err]
        for r in range(nr):
            if active[r]:
                compute_flux(fs[r], _di, bc, rheology)
                update_T(fs[r], _di, _dt, rheology)
                thermal_bcs(fs[r]["T"], bc)
        left = {r: fs[r]["T"].copy() for r in range(nr) if not active[r]}
        _blocks.exchange([[f["T"]] for f in fs], n, carts, L)
        for r, T in left.items():
            fs[r]["T"][...] = T
        it += 1
        for r in range(nr):
            if active[r]:
                done[r] = it
        if it % nout == 0:
            for r in range(nr):
                if active[r]:
                    check_res(fs[r], _di, _dt, rheology)
                    err[r] = np.sqrt((fs[r]["ResT"] * fs[r]["ResT"]).sum()) * _sq
                    norm_ResT[r].append(err[r])
                    iter_count[r].append(it)
            if stop == "max":
                err = [max(err)] * nr
            else:
                assert stop == "local", stop
    for f in fs:
        f["dT"][...] = f["T"] - f["Told"]
    return [dict(iter_count=np.array(iter_count[r], dtype=np.int64), norm_ResT=np.array(norm_ResT[r], dtype=fs[r]["T"].dtype), iterations=done[r]) for r in range(nr)]


def as_dtype(arrays, dtype):
    return {k: np.array(v, dtype=dtype, order="F") for k, v in arrays.items()}


# ------------------------------------------------------------------------------------------------ inputs and cases of the two test files
KYR = 1.0e3 * 3600 * 24 * 365.25
DT = 50 * KYR
LI = (100.0e3, 73.0e3, 131.0e3)                  # three different lengths
RHEOLOGY = dict(k=3.0, Cp=1.2e3, rho0=3.1e3, alpha=1.5e-5, T0=0.0)
TOL_ITERS, TOL_FLOOR, TOL_FACTOR = 1e-9, 1e-13, 100.0
# the four kinds a face can take: constant Value, No flux, constant Flux, nOthing; Latin square L<r>: face number k takes KINDS[(k + r) % 4], so that over
# L0 .. L3 every face has had every kind.  P<axis>: that pair periodic, the other faces as in L0 .. L2.
KINDS = "VNFO"
VALUES = dict(left=1650.0, right=1800.0, front=1700.0, back=1750.0, top=1600.0, bot=1900.0)
FLUX_FRACTION = dict(left=0.3, right=-0.2, front=0.15, back=-0.35, top=0.25, bot=-0.1)      # of K ΔT / d on that axis


def shapes(ni):
    nd = len(ni)
    c, g = tuple(ni), tuple(n + 2 for n in ni)
    s = {k: c for k in ("H", "shear_heating", "ResT", "K", "rhoCp", "thetar_dtau", "dtau_rho")}
    s.update(T=g, Told=g, dT=g)
    for ax in range(nd):
        s[QNAMES[ax]] = s[QNAMES[ax] + "2"] = tuple(n + (1 if a == ax else 0) for a, n in enumerate(ni))
    return s


def boundary_conditions(nd, name, _di):
    """SimpleNamespace(no_flux, constant_value, constant_flux, periodic): dictionaries over the faces of the dimension"""
    faces = FACES[nd]
    bc = SimpleNamespace(**{k: {f: False for f in faces} for k in ("no_flux", "constant_value", "constant_flux", "periodic")})
    periodic = ()
    if name[0] == "P":
        ax = "xyz".index(name[1])
        periodic = tuple(f for f in faces if AXIS[nd][f][0] == ax)
        r = ax
    else:
        r = int(name[1])
    for k, f in enumerate(faces):
        kind = KINDS[(k + r) % 4]
        if f in periodic:
            bc.periodic[f] = True
        elif kind == "V":
            bc.constant_value[f] = VALUES[f]
        elif kind == "N":
            bc.no_flux[f] = True
        elif kind == "F":
            bc.constant_flux[f] = FLUX_FRACTION[f] * 3.5 * 300.0 * _di[AXIS[nd][f][0]]
    return bc


def converging_bcs(nd):
    """no flux on the side faces, constant values on top and bot: without a constant-flux face (which keeps the qT*2 it holds) the residual of the loop goes to zero"""
    bc = SimpleNamespace(**{k: {f: False for f in FACES[nd]} for k in ("no_flux", "constant_value", "constant_flux", "periodic")})
    for f in FACES[nd]:
        if f in ("top", "bot"):
            bc.constant_value[f] = VALUES[f]
        else:
            bc.no_flux[f] = True
    return bc


def eps_between(a, b, start=1):
    """(ϵ, first check with min <= ϵ, first check with max <= ϵ), 0-based: ϵ half-way between the two ranks' norms at the first check from `start` on where they differ;
    asserts that the lower norm gets under ϵ strictly before the higher one does, which is what makes ϵ tell the two stop rules apart"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    k = next(i for i in range(start, len(a)) if a[i] != b[i])
    eps = float(0.5 * (a[k] + b[k]))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert (lo <= eps).any() and (hi <= eps).any(), (eps, list(lo), list(hi))
    first_min, first_max = int(np.argmax(lo <= eps)), int(np.argmax(hi <= eps))
    assert first_min < first_max, (eps, first_min, first_max)
    return eps, first_min, first_max


def make_inputs(ni, bc_name, seed):
    """random fields of the issue's ranges on a grid whose spacings all differ; θr_dτ and dτ_ρ are left zero (the caller fills them from PTThermalCoeffs)"""
    nd = len(ni)
    li = LI[:nd]
    di = tuple(l / n for l, n in zip(li, ni))
    assert len(set(di)) == nd, di
    _di = tuple(1.0 / d for d in di)
    rng = np.random.default_rng(seed)
    sh = shapes(ni)
    a = {k: np.zeros(s, order="F") for k, s in sh.items()}
    a["K"][...] = rng.uniform(2.0, 5.0, sh["K"])
    a["rhoCp"][...] = 3.96e6 * rng.uniform(0.7, 1.3, sh["rhoCp"])
    a["H"][...] = 1.0e-6 * rng.uniform(0.0, 2.0, sh["H"])
    a["shear_heating"][...] = 1.0e-7 * rng.uniform(0.0, 2.0, sh["H"])
    a["T"][...] = 1600.0 + 300.0 * rng.uniform(0.0, 1.0, sh["T"])
    for ax in range(nd):
        for suffix in ("", "2"):         # qT*2 too: a constant-flux face must keep what it holds
            a[QNAMES[ax] + suffix][...] = 3.5 * 300.0 * _di[ax] * rng.uniform(-1.0, 1.0, sh[QNAMES[ax]])
    return SimpleNamespace(ni=tuple(ni), li=li, di=di, _di=_di, dt=DT, CFL=0.95 / np.sqrt(nd + 0.1), arrays=a, bc=boundary_conditions(nd, bc_name, _di))


def observed(iterMax, nout):
    """1-based numbers of the iterations somebody observes: every check and the last one"""
    return sorted(set(range(nout, iterMax + 1, nout)) | {iterMax})


def expected_fused(iterMax, nout):
    return iterMax - len(observed(iterMax, nout))


def expected_replays(iterMax, nout, git=32):
    """graph launches of the loops: every run of unobserved iterations is replayed in whole graphs of `git` iterations"""
    n, last = 0, 0
    for o in observed(iterMax, nout):
        n += (o - 1 - last) // git
        last = o
    return n


def restate(inp, form, iterMax, nout, dtype):
    f = as_dtype(inp.arrays, dtype)
    r = heatdiffusion_PT(f, inp.bc, inp._di, inp.dt, iterMax=iterMax, nout=nout, rheology=RHEOLOGY if form == "rheology" else None)
    return f, r


def oracle_solve(oracle, inp, form, iterMax, nout):
    nd = len(inp.ni)
    params = oracle.thermal_params2d if nd == 2 else oracle.thermal_params3d
    p = params(inp.ni, inp._di, inp.dt, 1e-30, iterMax=iterMax, nout=nout, no_flux=inp.bc.no_flux, constant_value=inp.bc.constant_value,
               constant_flux=inp.bc.constant_flux, periodic=inp.bc.periodic, rheology=RHEOLOGY if form == "rheology" else None)
    ref = {k: v.copy(order="F") for k, v in inp.arrays.items()}
    r = (oracle.heatdiffusion_PT2d if nd == 2 else oracle.heatdiffusion_PT3d)(ref, p)
    return ref, r


def compared_fields(nd):
    return ("T", "Told", "dT", "ResT") + QNAMES[:nd] + tuple(q + "2" for q in QNAMES[:nd])


def _yardstick_of(fl, rl, fd, rd, _di, dt, rheo):
    """the rule in one place: per field the scale (maximum in the longdouble run; ResT: at least its largest term) and the bound TOL_FACTOR x the distance of the float64
    run from the longdouble one, at least TOL_FLOOR, at most TOL_ITERS; the norm history relative to itself"""
    scale, bound = {}, {}
    for k in compared_fields(fl["T"].ndim):
        scale[k] = float(np.abs(fl[k]).max())
        if k == "ResT":
            scale[k] = max(scale[k], res_term_scale(fl, _di, dt, rheo))
        bound[k] = min(max(TOL_FACTOR * float(np.abs(fd[k] - fl[k]).max()) / scale[k], TOL_FLOOR), TOL_ITERS)
    d = float(np.abs((rd["norm_ResT"] - rl["norm_ResT"]) / rl["norm_ResT"]).max()) if len(rl["norm_ResT"]) else 0.0
    bound["norm_ResT"] = min(max(TOL_FACTOR * d, TOL_FLOOR), TOL_ITERS)
    return SimpleNamespace(fields=fl, result=rl, scale=scale, bound=bound, float64=fd)


def yardstick(inp, form, iterMax, nout):
    """the longdouble restatement of a case, the scale of every compared field and its bound: TOL_FACTOR x the distance of the float64 restatement from the
    longdouble one, at least TOL_FLOOR, at most TOL_ITERS -- from the reference's formulas alone"""
    rheo = RHEOLOGY if form == "rheology" else None
    fl, rl = restate(inp, form, iterMax, nout, np.longdouble)
    fd, rd = restate(inp, form, iterMax, nout, np.float64)
    assert list(rl["iter_count"]) == list(rd["iter_count"]) == list(range(nout, iterMax + 1, nout))
    return _yardstick_of(fl, rl, fd, rd, inp._di, inp.dt, rheo)


def yardstick_blocks(blocks, bc, _di, dt, n, carts, L, form, iterMax, nout):
    """yardstick for every block of a decomposed case: blocks[r] = that rank's input dictionary (float64); the same rule, block by block, against
    heatdiffusion_PT_blocks in longdouble.  The result of rank r works with ratios_to_bound like the one of yardstick."""
    rheo = RHEOLOGY if form == "rheology" else None
    fl, fd = [as_dtype(b, np.longdouble) for b in blocks], [as_dtype(b, np.float64) for b in blocks]
    rl = heatdiffusion_PT_blocks(fl, bc, _di, dt, n, carts, L, iterMax=iterMax, nout=nout, rheology=rheo)
    rd = heatdiffusion_PT_blocks(fd, bc, _di, dt, n, carts, L, iterMax=iterMax, nout=nout, rheology=rheo)
    for r in range(len(blocks)):
        assert list(rl[r]["iter_count"]) == list(rd[r]["iter_count"]) == list(range(nout, iterMax + 1, nout))
    return [_yardstick_of(fl[r], rl[r], fd[r], rd[r], _di, dt, rheo) for r in range(len(blocks))]


def ratios_to_bound(got, result, y):
    """{field: distance from the longdouble restatement / bound}; the caller prints them and asserts that none exceeds 1"""
    out = {}
    for k, b in y.bound.items():
        if k == "norm_ResT":
            d = float(np.abs((np.asarray(result["norm_ResT"], dtype=np.longdouble) - y.result["norm_ResT"]) / y.result["norm_ResT"]).max()) if len(y.result["norm_ResT"]) else 0.0
        else:
            assert got[k].shape == y.fields[k].shape and np.isfinite(got[k]).all(), k
            d = float(np.abs(got[k].astype(np.longdouble) - y.fields[k]).max()) / y.scale[k]
        out[k] = d / b
    return out


# (id, ni, boundary conditions, (iterMax, nout), coefficient form); what each case is for is tabulated in tests/test_gpu_heat_diffusion_inputs.py
CASES2D = [
    ("2x2", (2, 2), "L0", (300, 100), "array"),
    ("3x130", (3, 130), "L1", (45, 20), "rheology"),
    ("63x5", (63, 5), "L2", (70, 7), "array"),
    ("64x9", (64, 9), "L3", (99, 33), "rheology"),
    ("65x33", (65, 33), "L0", (99, 33), "array"),
    ("127x4", (127, 4), "L1", (300, 100), "array"),
    ("128x6", (128, 6), "L2", (45, 20), "rheology"),
    ("128x6b", (128, 6), "L3", (70, 7), "array"),
    ("129x7", (129, 7), "L3", (300, 100), "array"),
    ("130x67", (130, 67), "L0", (70, 7), "rheology"),
    ("257x5", (257, 5), "L1", (99, 33), "array"),
    ("300x130", (300, 130), "L2", (45, 20), "array"),
    ("65x33px", (65, 33), "Px", (45, 20), "array"),
    ("129x7py", (129, 7), "Py", (99, 33), "rheology"),
]
CASES3D = [
    ("2x2x2", (2, 2, 2), "L0", (300, 100), "array"),
    ("20x9x7", (20, 9, 7), "L1", (45, 20), "rheology"),
    ("64x8x5", (64, 8, 5), "L2", (70, 7), "array"),
    ("65x16x6", (65, 16, 6), "L3", (99, 33), "rheology"),
    ("130x5x9", (130, 5, 9), "L0", (45, 20), "array"),
    ("20x9x7px", (20, 9, 7), "Px", (45, 20), "array"),
    ("20x9x7py", (20, 9, 7), "Py", (70, 7), "rheology"),
    ("20x9x7pz", (20, 9, 7), "Pz", (99, 33), "array"),
]


def case_seed(case_id):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(case_id))
