// stokes2d.hip -- 2D visco-elastic pseudo-transient Stokes path for gfx950.
//
// Reference being replaced: src/stokes/Stokes2D.jl:181-325 and its kernels
// (VelocityKernels.jl:3-6,10-44,108-131,246-269; PressureKernels.jl:10-15,186-195;
// StressKernels.jl:63-91; MiniKernels.jl:76-80; boundaryconditions/*.jl).  Same two-sweep fusion as
// the 3D path; at the reference's 2D sizes (<= 1024^2) the working set is Infinity-Cache resident,
// so these kernels are launch/latency bound rather than HBM bound.
// The 2D visco-elasto-plastic and non-linear drivers are in stokes2d_vep.hip; what they share with this file: stokes2d_kernels.hpp (device side), jrx2d_* (host side).
#include "jrx_internal.hpp"
#include "jrx_kernels.hpp"
#include "jrx_material.hpp"
#include "stokes2d_kernels.hpp"

namespace {

#define VX(i_, j_) Vx[(i_) + (i64)(nx + 1) * (j_)]
#define VY(i_, j_) Vy[(i_) + (i64)(nx + 2) * (j_)]
#define CC(i_, j_) ((i_) + (i64)nx * (j_))

template <bool DIAG>
__global__ __launch_bounds__(256) void k_stress2d(const Args2 a)
{
    const int nx = a.nx, ny = a.ny;
    const int t = xcd_slab_block() * blockDim.x + threadIdx.x;
    const int j = t / (nx + 1), i = t - j * (nx + 1);
    if (j > ny) return;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy, *__restrict__ eta = a.f.eta, *__restrict__ G = a.f.G;
    const double dt = a.dt, th = a.theta_dtau;
    if (i < nx && j < ny) {
        const i64 c = CC(i, j);
        const double dxi = (-VX(i, j + 1) + VX(i + 1, j + 1)) * spc(a.sp.vx, i, a._dx);
        const double dyi = (-VY(i + 1, j) + VY(i + 1, j + 1)) * spc(a.sp.vy, j, a._dy);
        const double divV = dxi + dyi;
        const double _Gdt = 1.0 / (G[c] * dt);
        {   // compute_P! with ητ (Stokes2D.jl:231-233)
            const double _Kdt = 1.0 / (a.f.K[c] * dt);
            const double _dt = 1.0 / dt;
            const double P = a.f.P[c], P0 = a.f.P0[c];
            const double rhs = -divV + (a.f.Q[c] * _dt);
            const double psi = 1.0 / (1.0 / a.etatau[c] + _Gdt) * a.r / th;
            a.f.P[c] = (fma(P0, _Kdt, rhs) * psi + P) / (1.0 + _Kdt * psi);
            if (DIAG) { a.f.RP[c] = fma(-(P - P0), _Kdt, rhs); a.f.divV[c] = divV; }
        }
        const double d3 = divV * (1.0 / 3.0);
        const double exx = dxi - d3, eyy = dyi - d3;
        if (DIAG) { a.f.exx[c] = exx; a.f.eyy[c] = eyy; }
        const double e = eta[c];
        const double dtr = dev_dtau_r(th, e, _Gdt);
        double tv;
        tv = a.f.txx[c]; a.f.txx[c] = tv + dev_stress_inc(tv, a.f.toxx[c], e, exx, _Gdt, dtr);
        tv = a.f.tyy[c]; a.f.tyy[c] = tv + dev_stress_inc(tv, a.f.toyy[c], e, eyy, _Gdt, dtr);
    }
    {   // vertex (i,j) of (nx+1, ny+1)
        const int im = max(i - 1, 0), ip = min(i, nx - 1), jm = max(j - 1, 0), jp = min(j, ny - 1);
        const double exy = 0.5 * (spc(a.sp.vxy, j, a._dy) * (VX(i, j + 1) - VX(i, j)) + spc(a.sp.vyx, i, a._dx) * (VY(i + 1, j) - VY(i, j)));
        const double e = 0.25 * (eta[CC(im, jm)] + eta[CC(ip, jm)] + eta[CC(im, jp)] + eta[CC(ip, jp)]);
        const double g = 0.25 * (G[CC(im, jm)] + G[CC(ip, jm)] + G[CC(im, jp)] + G[CC(ip, jp)]);
        const double _Gdt = 1.0 / (g * dt);
        const double dtr = dev_dtau_r(th, e, _Gdt);
        const i64 v = i + (i64)(nx + 1) * j;
        const double tv = a.f.txy[v];
        a.f.txy[v] = tv + dev_stress_inc(tv, a.f.toxy[v], e, exy, _Gdt, dtr);
        if (DIAG) a.f.exy[v] = exy;
    }
}

// ------------------------------------------------------------------------------------------------
// One PT iteration in one launch for iterations nobody observes (the 2D loop is launch-bound): compute_V! of iteration m, flow_bcs! by
// rule, and compute_∇V! / compute_P! / compute_strain_rate! / compute_τ! of iteration m+1, reading the state (P, τ, V) from one set and
// writing it to the other.  A thread owns node (i, j) of the (nx+1) x (ny+1) node grid: it computes the new velocities of its cell and
// of the cell below (the row below recomputes them for itself), takes those of the column to its left from the neighbouring lane
// (waves overlap by one lane: lane 0 only feeds lane 1), derives boundary and ghost entries from the flow_bcs! rules, and then does
// the stress update of its cell centre and its vertex exactly as k_stress2d does.  Same arithmetic, in the same order.
// ------------------------------------------------------------------------------------------------
struct Out6_2d { double *P, *txx, *tyy, *txy, *Vx, *Vy; };
struct BC2 { int tL, tR, tB, tT; };      // 0 none (memory holds the prescribed value), 1 free slip, 2 no slip; B: j = 1, T: j = end
__global__ __launch_bounds__(256) void k_fused2d(const Args2 a, const Out6_2d o, const BC2 bc, const int nwx)
{
    const int nx = a.nx, ny = a.ny;
    const int wg = (int)xcd_slab_block() * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int j = wg / nwx, i = (wg - j * nwx) * 63 + lane - 1;
    if (j > ny) return;
    const double _dx = a._dx, _dy = a._dy, edt = a.eta_dtau, dt = a.dt, th = a.theta_dtau;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy, *__restrict__ P = a.f.P, *__restrict__ et = a.etatau;
    const double *__restrict__ txy = a.f.txy, *__restrict__ eta = a.f.eta, *__restrict__ G = a.f.G;
#define TXY(i_, j_) txy[(i_) + (i64)(nx + 1) * (j_)]
    // compute_V! of cell (ci, cj): the new Vx[ci+1, cj+1] and Vy[ci+1, cj+1]; nodes on the right / top boundary planes keep their value
    auto Bcell = [&](const int ci, const int cj, double &vx_, double &vy_) {
        const i64 c = CC(ci, cj);
        const double Pc = P[c], ec = et[c];
        if (ci < nx - 1) {
            const double dP = (-Pc + P[c + 1]) * _dx, dT = (-a.f.txx[c] + a.f.txx[c + 1]) * _dx;
            const double dS = (-TXY(ci + 1, cj) + TXY(ci + 1, cj + 1)) * _dy, av = (a.f.fx[c] + a.f.fx[c + 1]) * 0.5;
            vx_ = VX(ci + 1, cj + 1) + (-dP + dT + dS - av) * edt / ((ec + et[c + 1]) * 0.5);
        } else vx_ = bc.tR == 2 ? 0.0 : VX(nx, cj + 1);
        if (cj < ny - 1) {
            const double dP = (-Pc + P[c + nx]) * _dy, dT = (-a.f.tyy[c] + a.f.tyy[c + nx]) * _dy;
            const double dS = (-TXY(ci, cj + 1) + TXY(ci + 1, cj + 1)) * _dx, av = (a.f.fy[c] + a.f.fy[c + nx]) * 0.5;
            vy_ = VY(ci + 1, cj + 1) + (-dP + dT + dS - av) * edt / ((ec + et[c + nx]) * 0.5);
        } else vy_ = bc.tT == 2 ? 0.0 : VY(ci + 1, ny);
    };
    auto rule = [](const int t, const double v, const double mem) { return t == 1 ? v : (t == 2 ? -v : mem); };
    const bool col = i >= 0 && i < nx;                 // this lane has a cell column
    double vxn = 0.0, vyn = 0.0, vxb = 0.0, vyb = 0.0;   // new Vx[i+1, j+1], Vy[i+1, j+1] (own row) and Vx[i+1, j], Vy[i+1, j] (row below)
    if (col) {
        if (j < ny) Bcell(i, j, vxn, vyn);
        if (j >= 1) Bcell(i, j - 1, vxb, vyb);
        else {
            vxb = rule(bc.tB, vxn, VX(i + 1, 0));                 // ghost row below the bottom face
            vyb = bc.tB == 2 ? 0.0 : VY(i + 1, 0);                // Vy on the bottom face
        }
        if (j == ny) vxn = rule(bc.tT, vxb, VX(i + 1, ny + 1));   // ghost row above the top face
    }
    const double Lvxn = __shfl_up(vxn, 1, 64), Lvxb = __shfl_up(vxb, 1, 64), Lvyb = __shfl_up(vyb, 1, 64);
    if (lane == 0 || i < 0 || i > nx) return;          // feeder lane / beyond the row
    // new velocities on the left of the node: Vx[i, j+1], Vx[i, j], Vy[i, j]
    double X1, X0, Y0;
    if (i >= 1) { X1 = Lvxn; X0 = Lvxb; Y0 = Lvyb; }
    else {
        // left boundary plane of Vx (ghost rows by the bottom / top rule) and ghost column of Vy
        auto VxL = [&](const int jr) -> double {
            const double lo = bc.tL == 2 ? 0.0 : VX(0, 1), hi = bc.tL == 2 ? 0.0 : VX(0, ny);
            if (jr == 0) return rule(bc.tB, lo, VX(0, 0));
            if (jr == ny + 1) return rule(bc.tT, hi, VX(0, ny + 1));
            return bc.tL == 2 ? 0.0 : VX(0, jr);
        };
        X1 = VxL(j + 1); X0 = VxL(j);
        Y0 = rule(bc.tL, vyb, VY(0, j));
    }
    const double Yr = i < nx ? vyb : rule(bc.tR, Lvyb, VY(nx + 1, j));        // Vy[i+1, j]; beyond the right face: ghost column
    if (i < nx && j < ny) {
        const i64 c = CC(i, j);
        const double dxi = (-X1 + vxn) * _dx;
        const double dyi = (-vyb + vyn) * _dy;
        const double divV = dxi + dyi;
        const double _Gdt = 1.0 / (G[c] * dt);
        {   // compute_P! with ητ (Stokes2D.jl:231-233)
            const double _Kdt = 1.0 / (a.f.K[c] * dt);
            const double _dt = 1.0 / dt;
            const double Pc = P[c], P0 = a.f.P0[c];
            const double rhs = -divV + (a.f.Q[c] * _dt);
            const double psi = 1.0 / (1.0 / et[c] + _Gdt) * a.r / th;
            o.P[c] = (fma(P0, _Kdt, rhs) * psi + Pc) / (1.0 + _Kdt * psi);
        }
        const double d3 = divV * (1.0 / 3.0);
        const double exx = dxi - d3, eyy = dyi - d3;
        const double e = eta[c];
        const double dtr = dev_dtau_r(th, e, _Gdt);
        double tv;
        tv = a.f.txx[c]; o.txx[c] = tv + dev_stress_inc(tv, a.f.toxx[c], e, exx, _Gdt, dtr);
        tv = a.f.tyy[c]; o.tyy[c] = tv + dev_stress_inc(tv, a.f.toyy[c], e, eyy, _Gdt, dtr);
        if (i < nx - 1) o.Vx[(i + 1) + (i64)(nx + 1) * (j + 1)] = vxn;
        if (j < ny - 1) o.Vy[(i + 1) + (i64)(nx + 2) * (j + 1)] = vyn;
    }
    {   // vertex (i, j)
        const int im = max(i - 1, 0), ip = min(i, nx - 1), jm = max(j - 1, 0), jp = min(j, ny - 1);
        const double exy = 0.5 * (_dy * (X1 - X0) + _dx * (Yr - Y0));
        const double e = 0.25 * (eta[CC(im, jm)] + eta[CC(ip, jm)] + eta[CC(im, jp)] + eta[CC(ip, jp)]);
        const double g = 0.25 * (G[CC(im, jm)] + G[CC(ip, jm)] + G[CC(im, jp)] + G[CC(ip, jp)]);
        const double _Gdt = 1.0 / (g * dt);
        const double dtr = dev_dtau_r(th, e, _Gdt);
        const i64 v = i + (i64)(nx + 1) * j;
        const double tv = txy[v];
        o.txy[v] = tv + dev_stress_inc(tv, a.f.toxy[v], e, exy, _Gdt, dtr);
    }
#undef TXY
}

// ------------------------------------------------------------------------------------------------
// k_fused2d with every operand requested up front (option "fused2d_batch", default).  The kernel above follows the reference's control flow -- compute_V! of the own cell,
// of the cell below, the boundary rules, compute_P!, compute_τ! of the centre, of the vertex -- and every `if` on the way ends a basic block, so its ~50 loads reach the
// memory system as a chain of 12-14 dependent groups: on the grids this kernel runs on (everything sits in L2 / Infinity Cache) an iteration IS that chain of round trips.
// Here the loads are unconditional (clamped indices; what a boundary lane does not use it does not use), issued as one batch and pinned ahead of the arithmetic; the
// arithmetic is the kernel above, expression for expression, with the boundary cases as selects.  VISC (dt = Inf, SolCx and every purely viscous 2D run): the seven arrays
// that only ever meet 1/(G dt), 1/(K dt), 1/dt -- τ_o (3), P0, K, G, Q -- are not loaded (finite operands: the driver checks them once per solve), as in 3D.
// ------------------------------------------------------------------------------------------------
template <bool VISC>
__global__ __launch_bounds__(256) void k_fused2d_b(const Args2 a, const Out6_2d o, const BC2 bc, const int nwx)
{
    const int nx = a.nx, ny = a.ny;
    const int wg = (int)xcd_slab_block() * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int j = wg / nwx, i = (wg - j * nwx) * 63 + lane - 1;
    if (j > ny) return;
    const double _dx = a._dx, _dy = a._dy, edt = a.eta_dtau, dt = a.dt, th = a.theta_dtau;
    const double *__restrict__ Vx = a.f.Vx, *__restrict__ Vy = a.f.Vy, *__restrict__ P = a.f.P, *__restrict__ et = a.etatau;
    const double *__restrict__ txy = a.f.txy, *__restrict__ eta = a.f.eta, *__restrict__ G = a.f.G;
    typedef unsigned int u32;
#define LB(p_, off_) (*(const double *)((const char *)(p_) + (off_)))
    // clamped cell column / rows: r0 = j - 1, r1 = j, r2 = j + 1 (cells), ip = ic + 1 (cells)
    const int ic = min(max(i, 0), nx - 1), ip = min(ic + 1, nx - 1);
    const int r0 = min(max(j - 1, 0), ny - 1), r1 = min(j, ny - 1), r2 = min(j + 1, ny - 1);
    const u32 c0 = 8u * (u32)(ic + nx * r0), c1 = 8u * (u32)(ic + nx * r1), c2 = 8u * (u32)(ic + nx * r2), dxp = 8u * (u32)(ip - ic);
    // node rows of τxy (nx+1 columns, rows 0..ny): j - 1, j, j + 1 clamped; node column ic + 1 and ic
    const int n0 = max(j - 1, 0), n2 = min(j + 1, ny);
    const u32 t0 = 8u * (u32)(ic + (nx + 1) * n0), t1 = 8u * (u32)(ic + (nx + 1) * j), t2 = 8u * (u32)(ic + (nx + 1) * n2);
    // Vx (nx+1 columns, rows 0..ny+1): (i+1, j), (i+1, j+1);  Vy (nx+2 columns, rows 0..ny): (i+1, j), (i+1, min(j+1, ny)).  The feeder lane of the first segment (i = -1) thereby
    // loads the boundary column Vx[0, ·], Vy[0, ·] for the lane on the left face, and the lane on the right face (i = nx, no cell of its own) the ghost column Vy[nx+1, j]
    const int cvx = min(max(i + 1, 0), nx), cvy = min(max(i + 1, 0), nx + 1);
    const u32 vx0 = 8u * (u32)(cvx + (nx + 1) * j), vx1 = vx0 + 8u * (u32)(nx + 1);
    const u32 vy0 = 8u * (u32)(cvy + (nx + 2) * j), vy1 = 8u * (u32)(cvy + (nx + 2) * n2);
    // vertex (i, j): the four cells around it, clamped
    const int iq = min(max(i, 0), nx - 1), jm = max(j - 1, 0), jq = min(j, ny - 1);
    const u32 v10 = 8u * (u32)(iq + nx * jm), v11 = 8u * (u32)(iq + nx * jq);
    const u32 vv = 8u * (u32)(min(max(i, 0), nx) + (nx + 1) * j);
    // ---- every operand
    const double P00 = LB(P, c0), P10 = LB(P, c0 + dxp), P01 = LB(P, c1), P11 = LB(P, c1 + dxp), P02 = LB(P, c2);
    const double E00 = LB(et, c0), E10 = LB(et, c0 + dxp), E01 = LB(et, c1), E11 = LB(et, c1 + dxp), E02 = LB(et, c2);
    const double X00 = LB(a.f.txx, c0), X10 = LB(a.f.txx, c0 + dxp), X01 = LB(a.f.txx, c1), X11 = LB(a.f.txx, c1 + dxp);
    const double Y00 = LB(a.f.tyy, c0), Y01 = LB(a.f.tyy, c1), Y02 = LB(a.f.tyy, c2);
    const double Fx00 = LB(a.f.fx, c0), Fx10 = LB(a.f.fx, c0 + dxp), Fx01 = LB(a.f.fx, c1), Fx11 = LB(a.f.fx, c1 + dxp);
    const double Fy00 = LB(a.f.fy, c0), Fy01 = LB(a.f.fy, c1), Fy02 = LB(a.f.fy, c2);
    const double S10 = LB(txy, t0 + 8u), S01 = LB(txy, t1), S11 = LB(txy, t1 + 8u), S02 = LB(txy, t2), S12 = LB(txy, t2 + 8u);     // τxy[ic+1, j-1], [ic, j], [ic+1, j], [ic, j+1], [ic+1, j+1]
    const double Ux0 = LB(Vx, vx0), Ux1 = LB(Vx, vx1), Uy0 = LB(Vy, vy0), Uy1 = LB(Vy, vy1);
    const double e10 = LB(eta, v10), e11 = LB(eta, v11);
    double g10 = 0, g11 = 0, Gc = 0, Kc = 0, P0c = 0, Qc = 0, toxx = 0, toyy = 0, toxy = 0;
    if (!VISC) {
        g10 = LB(G, v10); g11 = LB(G, v11);
        Gc = g11;          // (where the centre is updated, i < nx and j < ny, the vertex's cell (iq, jq) is the own cell)
    }
    const double ec1 = e11, tvv = i < nx ? S01 : S11;       // η of the own cell = the vertex's (iq, jq); τxy[i, j]: the own node column, or the last one (ic + 1 = nx)
    __builtin_amdgcn_sched_barrier(0);
    // ---- compute_V! of cell (ci, cj) from its operands: Pc, P[c+1], P[c+nx], ... (k_fused2d::Bcell)
    auto Bcell = [&](const int ci, const int cj, const double Pc, const double Px, const double Py, const double ec, const double ex, const double ey, const double txc,
                     const double txr, const double tyc, const double tyu, const double s_r0, const double s_r1, const double s_l1, const double fxc, const double fxr,
                     const double fyc, const double fyu, const double vxo, const double vyo, double &vx_, double &vy_) {
        if (ci < nx - 1) {
            const double dP = (-Pc + Px) * _dx, dT = (-txc + txr) * _dx;
            const double dS = (-s_r0 + s_r1) * _dy, av = (fxc + fxr) * 0.5;
            vx_ = vxo + (-dP + dT + dS - av) * edt / ((ec + ex) * 0.5);
        } else vx_ = bc.tR == 2 ? 0.0 : vxo;
        if (cj < ny - 1) {
            const double dP = (-Pc + Py) * _dy, dT = (-tyc + tyu) * _dy;
            const double dS = (-s_l1 + s_r1) * _dx, av = (fyc + fyu) * 0.5;
            vy_ = vyo + (-dP + dT + dS - av) * edt / ((ec + ey) * 0.5);
        } else vy_ = bc.tT == 2 ? 0.0 : vyo;
    };
    auto rule = [](const int t, const double v, const double mem) { return t == 1 ? v : (t == 2 ? -v : mem); };
    const bool col = i >= 0 && i < nx;
    double vxn = 0.0, vyn = 0.0, vxb = 0.0, vyb = 0.0;
    if (col) {
        //                         Pc   P[c+1] P[c+nx] ec  e[c+1] e[c+nx] txx  txx+1 tyy  tyy+nx τxy[ci+1,cj] [ci+1,cj+1] [ci,cj+1]
        if (j < ny) Bcell(i, j, P01, P11, P02, E01, E11, E02, X01, X11, Y01, Y02, S11, S12, S02, Fx01, Fx11, Fy01, Fy02, Ux1, Uy1, vxn, vyn);
    }
    if (!VISC) {
        // the six operands only the stress update reads, requested once the first compute_V! has consumed its share of the batch (the register peak that decides between four
        // and five waves per SIMD -- 512^2 is 4,617 waves for 4,096 or 5,120 slots) and pinned here: in flight under the second compute_V! and the lane exchanges
        __builtin_amdgcn_sched_barrier(0);
        Kc = LB(a.f.K, c1); P0c = LB(a.f.P0, c1); Qc = LB(a.f.Q, c1); toxx = LB(a.f.toxx, c1); toyy = LB(a.f.toyy, c1); toxy = LB(a.f.toxy, vv);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (col) {
        if (j >= 1) Bcell(i, j - 1, P00, P10, P01, E00, E10, E01, X00, X10, Y00, Y01, S10, S11, S01, Fx00, Fx10, Fy00, Fy01, Ux0, Uy0, vxb, vyb);
        else {
            vxb = rule(bc.tB, vxn, Ux0);                 // ghost row below the bottom face: Vx[i+1, 0]
            vyb = bc.tB == 2 ? 0.0 : Uy0;                // Vy on the bottom face: Vy[i+1, 0]
        }
        if (j == ny) vxn = rule(bc.tT, vxb, Ux1);        // ghost row above the top face: Vx[i+1, ny+1]
    }
    const double Lvxn = __shfl_up(vxn, 1, 64), Lvxb = __shfl_up(vxb, 1, 64), Lvyb = __shfl_up(vyb, 1, 64);
    // from the lane to the left: its velocity loads (for the lane on the left face: the boundary column) and the vertex's two left-hand cells (im, jm), (im, jq) = that lane's (iq, jm), (iq, jq)
    const double LUx0 = __shfl_up(Ux0, 1, 64), LUx1 = __shfl_up(Ux1, 1, 64), LUy0 = __shfl_up(Uy0, 1, 64);
    const double Le10 = __shfl_up(e10, 1, 64), Le11 = __shfl_up(e11, 1, 64);
    const double e00 = i > 0 ? Le10 : e10, e01 = i > 0 ? Le11 : e11;
    double g00 = 0, g01 = 0;
    if (!VISC) {
        const double Lg10 = __shfl_up(g10, 1, 64), Lg11 = __shfl_up(g11, 1, 64);
        g00 = i > 0 ? Lg10 : g10; g01 = i > 0 ? Lg11 : g11;
    }
    if (lane == 0 || i < 0 || i > nx) return;          // feeder lane / beyond the row
    const double B0 = LUx0, B1 = LUx1, BY = i == 0 ? LUy0 : Uy0;      // i = 0: Vx[0, j], Vx[0, j+1], Vy[0, j];  i = nx: Vy[nx+1, j]
    double X1, X0, Y0;
    if (i >= 1) { X1 = Lvxn; X0 = Lvxb; Y0 = Lvyb; }
    else {
        // left boundary plane of Vx (ghost rows by the bottom / top rule) and ghost column of Vy: B0 = Vx[0, j], B1 = Vx[0, j+1], BY = Vy[0, j]
        const double b0 = bc.tL == 2 ? 0.0 : B0, b1 = bc.tL == 2 ? 0.0 : B1;
        X1 = (j + 1 == ny + 1) ? rule(bc.tT, b0, B1) : b1;
        X0 = (j == 0) ? rule(bc.tB, b1, B0) : b0;
        Y0 = rule(bc.tL, vyb, BY);
    }
    const double Yr = i < nx ? vyb : rule(bc.tR, Lvyb, BY);        // Vy[i+1, j]; beyond the right face: ghost column Vy[nx+1, j]
    if (i < nx && j < ny) {
        const double dxi = (-X1 + vxn) * _dx;
        const double dyi = (-vyb + vyn) * _dy;
        const double divV = dxi + dyi;
        const double _Gdt = VISC ? 0.0 : 1.0 / (Gc * dt);
        {   // compute_P! with ητ (Stokes2D.jl:231-233)
            const double _Kdt = VISC ? 0.0 : 1.0 / (Kc * dt);
            const double _dt = 1.0 / dt;
            const double rhs = -divV + (Qc * _dt);
            const double psi = 1.0 / (1.0 / E01 + _Gdt) * a.r / th;
            *(double *)((char *)o.P + c1) = (fma(P0c, _Kdt, rhs) * psi + P01) / (1.0 + _Kdt * psi);
        }
        const double d3 = divV * (1.0 / 3.0);
        const double exx = dxi - d3, eyy = dyi - d3;
        const double dtr = dev_dtau_r(th, ec1, _Gdt);
        *(double *)((char *)o.txx + c1) = X01 + dev_stress_inc(X01, toxx, ec1, exx, _Gdt, dtr);
        *(double *)((char *)o.tyy + c1) = Y01 + dev_stress_inc(Y01, toyy, ec1, eyy, _Gdt, dtr);
        if (i < nx - 1) o.Vx[(i + 1) + (i64)(nx + 1) * (j + 1)] = vxn;
        if (j < ny - 1) o.Vy[(i + 1) + (i64)(nx + 2) * (j + 1)] = vyn;
    }
    {   // vertex (i, j)
        const double exy = 0.5 * (_dy * (X1 - X0) + _dx * (Yr - Y0));
        const double e = 0.25 * (e00 + e10 + e01 + e11);
        const double g = 0.25 * (g00 + g10 + g01 + g11);
        const double _Gdt = VISC ? 0.0 : 1.0 / (g * dt);
        const double dtr = dev_dtau_r(th, e, _Gdt);
        *(double *)((char *)o.txy + vv) = tvv + dev_stress_inc(tvv, toxy, e, exy, _Gdt, dtr);
    }
#undef LB
}

// dt = Inf (see k_fused2d_b<VISC>): one streaming pass checks that every entry of the arrays the viscous-limit form does not load is harmless -- τ_o, P0, Q finite, K and G neither
// NaN nor 0 (0 * Inf) -- as visc_operands_check does in 3D; if not, the general form runs and produces the reference's NaNs
__global__ __launch_bounds__(256) void k_visc_operands_ok2d(const double *__restrict__ P0, const double *__restrict__ Q, const double *__restrict__ toxx, const double *__restrict__ toyy,
                                                            const double *__restrict__ K, const double *__restrict__ G, i64 nc, const double *__restrict__ toxy, i64 nv, int *bad)
{
    const i64 stride = (i64)gridDim.x * blockDim.x;
    bool b = false;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < nv; t += stride) {
        if (t < nc) {
            b |= !(isfinite(P0[t]) && isfinite(Q[t]) && isfinite(toxx[t]) && isfinite(toyy[t]));
            const double k = K[t], g = G[t];
            b |= (k != k) || (g != g) || k == 0.0 || g == 0.0;
        }
        b |= !isfinite(toxy[t]);
    }
    if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}
#undef VX
#undef VY
#undef CC

}   // namespace

// ---- host pieces that the 2D VEP drivers (stokes2d_vep.hip) reuse, declared in jrx_internal.hpp

// the six inverse-spacing arrays of a non-uniform grid come together or not at all
bool jrx2d_spacing_ok(const double *const sp[6])
{
    int n = 0;
    for (int q = 0; q < 6; q++) n += sp[q] != nullptr;
    return n == 0 || n == 6;
}

jrx_status jrx2d_bcs(jrx_handle *h, hipStream_t s, double *Vx, double *Vy, int nx, int ny, uint32_t fs, uint32_t ns, uint32_t pe)
{
    BcArr A[3] = {{Vx, {nx + 1, ny + 2, 1}}, {Vy, {nx + 2, ny + 1, 1}}, {nullptr, {0, 0, 0}}};
    auto run = [&](int type, int dim, bool lo, bool hi) -> jrx_status {
        if (!lo && !hi) return JRX_OK;
        const int d1 = dim == 0 ? 1 : 0;
        const int na = A[0].n[d1] > A[1].n[d1] ? A[0].n[d1] : A[1].n[d1];
        hipLaunchKernelGGL(k_bc3d, dim3((na + 255) / 256, 1), dim3(256), 0, s, A[0], A[1], A[2], type, dim, (int)lo, (int)hi);
        JRX_LAUNCH_CHECK(h);
        return JRX_OK;
    };
    // 2D naming: bot <-> j = 1, top <-> j = end for every condition (no_slip.jl:1-18, free_slip.jl:1-13, periodic.jl:15-36)
    if (ns) {
        JRX_TRY(run(1, 0, ns & JRX_FACE_LEFT, ns & JRX_FACE_RIGHT));
        JRX_TRY(run(1, 1, ns & JRX_FACE_BOT, ns & JRX_FACE_TOP));
    }
    if (fs) {
        JRX_TRY(run(0, 1, fs & JRX_FACE_BOT, fs & JRX_FACE_TOP));
        JRX_TRY(run(0, 0, fs & JRX_FACE_LEFT, fs & JRX_FACE_RIGHT));
    }
    if (pe) {
        JRX_TRY(run(2, 0, pe & JRX_FACE_LEFT, pe & JRX_FACE_RIGHT));
        JRX_TRY(run(2, 1, pe & JRX_FACE_BOT, pe & JRX_FACE_TOP));
    }
    return JRX_OK;
}

jrx_status jrx2d_sumsq(jrx_handle *h, hipStream_t s, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p)
{
    const int nx = (int)p->nx, ny = (int)p->ny;
    RedArr A0 = {f->Rx, {nx - 1, ny, 1}, 1}, A1 = {f->Ry, {nx, ny - 1, 1}, 1}, A2 = {nullptr, {0, 0, 0}, 0}, A3 = {f->RP, {nx, ny, 1}, 0};
    int nb = (int)(((i64)nx * ny + 2047) / 2048);
    nb = nb < 1 ? 1 : (nb > kMaxRedBlocks ? kMaxRedBlocks : nb);
    hipLaunchKernelGGL(k_sumsq_partial, dim3(nb), dim3(256), 0, s, A0, A1, A2, A3, h->d_partials);
    JRX_LAUNCH_CHECK(h);
    hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, s, h->d_partials, nb, h->d_sums);
    JRX_LAUNCH_CHECK(h);
    return JRX_OK;
}

namespace {

jrx_status check2(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p)
{
    if (!h) return JRX_ERR_ARG;
    if (!f || !p) return jrx_fail(h, JRX_ERR_ARG, "null fields/params");
    JRX_TRY(jrx_check_device(h));
    if (p->nx < 3 || p->ny < 3) return jrx_fail(h, JRX_ERR_ARG, "2D Stokes needs at least 3 cells per dimension");
    if ((double)(p->nx + 2) * (double)(p->ny + 2) >= 2147483647.0) return jrx_fail(h, JRX_ERR_UNSUPPORTED, "grid too large");
    const void *req[] = {f->P, f->P0, f->divV, f->Q, f->Vx, f->Vy, f->Ux, f->Uy, f->txx, f->tyy, f->txy, f->toxx, f->toyy, f->toxy,
                         f->exx, f->eyy, f->exy, f->eta, f->K, f->G, f->fx, f->fy, f->RP, f->Rx, f->Ry};
    for (const void *q : req)
        if (!q) return jrx_fail(h, JRX_ERR_ARG, "a required 2D field pointer is NULL");
    if (!jrx2d_spacing_ok(p->inv_spacing)) return jrx_fail(h, JRX_ERR_ARG, "non-uniform grid: all six inverse-spacing arrays are required");
    return JRX_OK;
}

// fuse_bc: flow_bcs! has already been applied in full once in this solve, nothing observes U in this iteration and no face is
// periodic, so the velocity kernel refreshes the ghosts itself
jrx_status enqueue_iteration2(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau, const jrx_stokes2d_params *p, bool diag,
                              bool fuse_bc, bool skip_stress, bool *bcs_full_done);
jrx_status enqueue_iteration2(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau, const jrx_stokes2d_params *p, bool diag,
                              bool fuse_bc = false)
{
    return enqueue_iteration2(h, f, etatau, p, diag, fuse_bc, false, nullptr);
}
// skip_stress: the stress sweep of this iteration has already been applied (by a fused launch); bcs_full_done (optional): set when
// flow_bcs! has been launched in full
jrx_status enqueue_iteration2(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau, const jrx_stokes2d_params *p, bool diag,
                              bool fuse_bc, bool skip_stress, bool *bcs_full_done)
{
    const int nx = (int)p->nx, ny = (int)p->ny;
    Args2 a = make_args2(f, etatau, p);
    hipStream_t s = h->stream;
    const unsigned gA = (unsigned)(((i64)(nx + 1) * (ny + 1) + 255) / 256), gB = (unsigned)(((i64)nx * ny + 255) / 256);
    if (!skip_stress) {
        if (diag) hipLaunchKernelGGL(k_stress2d<true>, dim3(gA), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_stress2d<false>, dim3(gA), dim3(256), 0, s, a);
        JRX_LAUNCH_CHECK(h);
    }
    if (fuse_bc && !diag && p->periodic == 0 && !jrx_comm_active(h) && !p->displacement_bcs) {
        hipLaunchKernelGGL((k_velocity2d<false, true>), dim3(gB), dim3(256), 0, s, a);
        JRX_LAUNCH_CHECK(h);
        return JRX_OK;
    }
    hipLaunchKernelGGL(k_velocity2d<false>, dim3(gB), dim3(256), 0, s, a);
    JRX_LAUNCH_CHECK(h);
    if (diag) {
        hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Ux, f->Vx, (i64)(nx + 1) * (ny + 2), f->Uy, f->Vy, (i64)(nx + 2) * (ny + 1),
                           (double *)nullptr, (const double *)nullptr, (i64)0, p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    if (p->displacement_bcs) {    // flow_bcs! on U = V dt (overwritten by the next iteration: only observable ones matter); V's ghosts stay as they are
        if (diag) JRX_TRY(jrx2d_bcs(h, s, f->Ux, f->Uy, nx, ny, p->free_slip, p->no_slip, p->periodic));
    } else {
        JRX_TRY(jrx2d_bcs(h, s, f->Vx, f->Vy, nx, ny, p->free_slip, p->no_slip, p->periodic));
        if (bcs_full_done) *bcs_full_done = true;
    }
    if (jrx_comm_active(h)) {
        double *arrs[2] = {f->Vx, f->Vy};
        const int64_t ext[2][3] = {{nx + 1, ny + 2, 1}, {nx + 2, ny + 1, 1}};
        const int64_t n[3] = {nx, ny, 1};
        JRX_TRY(jrx_halo_exchange(h, s, 2, arrs, ext, n));
    }
    return JRX_OK;
}

}   // namespace

extern "C" {

jrx_status jrx_stokes2d_sweep_stress(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau, const jrx_stokes2d_params *p, int32_t flags)
{
    JRX_TRY(check2(h, f, p));
    if (!etatau) return jrx_fail(h, JRX_ERR_ARG, "etatau is NULL");
    Args2 a = make_args2(f, etatau, p);
    const unsigned gA = (unsigned)(((i64)(p->nx + 1) * (p->ny + 1) + 255) / 256);
    if (flags & JRX_OUT_DIAG) hipLaunchKernelGGL(k_stress2d<true>, dim3(gA), dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL(k_stress2d<false>, dim3(gA), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_stokes2d_sweep_velocity(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau, const jrx_stokes2d_params *p, int32_t flags)
{
    JRX_TRY(check2(h, f, p));
    if (!etatau) return jrx_fail(h, JRX_ERR_ARG, "etatau is NULL");
    Args2 a = make_args2(f, etatau, p);
    const unsigned gB = (unsigned)(((i64)p->nx * p->ny + 255) / 256);
    hipLaunchKernelGGL(k_velocity2d<false>, dim3(gB), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    if (flags & JRX_OUT_DIAG) {
        hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, h->stream, f->Ux, f->Vx, (i64)(p->nx + 1) * (p->ny + 2), f->Uy, f->Vy,
                           (i64)(p->nx + 2) * (p->ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_stokes2d_compute_res(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p)
{
    JRX_TRY(check2(h, f, p));
    Args2 a = make_args2(f, nullptr, p);
    const unsigned gB = (unsigned)(((i64)p->nx * p->ny + 255) / 256);
    hipLaunchKernelGGL(k_velocity2d<true>, dim3(gB), dim3(256), 0, h->stream, a);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_flow_bcs2d(jrx_handle *h, double *Vx, double *Vy, int64_t nx, int64_t ny, uint32_t free_slip, uint32_t no_slip, uint32_t periodic)
{
    if (!h) return JRX_ERR_ARG;
    if (!Vx || !Vy) return jrx_fail(h, JRX_ERR_ARG, "null velocity pointer");
    JRX_TRY(jrx2d_bcs(h, h->stream, Vx, Vy, (int)nx, (int)ny, free_slip, no_slip, periodic));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

jrx_status jrx_stokes2d_residual_sumsq(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p, double out[3])
{
    JRX_TRY(check2(h, f, p));
    JRX_TRY(jrx2d_sumsq(h, h->stream, f, p));
    JRX_HIP(h, hipMemcpyAsync(h->h_sums, h->d_sums, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    out[0] = h->h_sums[0]; out[1] = h->h_sums[1]; out[2] = h->h_sums[3];
    return JRX_OK;
}

jrx_status jrx_stokes2d_solve(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p, jrx_solve_result *res)
{
    JRX_TRY(check2(h, f, p));
    if (!res) return jrx_fail(h, JRX_ERR_ARG, "null result");
    if (p->nout < 1) return jrx_fail(h, JRX_ERR_ARG, "nout must be >= 1");
    const int nx = (int)p->nx, ny = (int)p->ny;
    const size_t n = (size_t)nx * ny;
    hipStream_t s = h->stream;
    JRX_TRY(jrx_ensure_etatau(h, n));
    // compute_maxloc!(ητ, η; window=(1,1)); update_halo!(ητ)   (Stokes2D.jl:206-210)
    hipLaunchKernelGGL(k_maxloc, dim3((unsigned)((n + 255) / 256), 1), dim3(256), 0, s, h->etatau, f->eta, nx, ny, 1);
    JRX_LAUNCH_CHECK(h);
    if (jrx_comm_active(h)) {
        double *arrs[1] = {h->etatau};
        const int64_t ext[1][3] = {{nx, ny, 1}};
        const int64_t nn[3] = {nx, ny, 1};
        JRX_TRY(jrx_halo_exchange(h, s, 1, arrs, ext, nn));
    }
    if (p->displacement_bcs) {    // displacement2velocity!(stokes, dt, flow_bcs) (Stokes2D.jl:223)
        hipLaunchKernelGGL(k_scale3, dim3(256), dim3(256), 0, s, f->Vx, (const double *)f->Ux, (i64)(nx + 1) * (ny + 2), f->Vy,
                           (const double *)f->Uy, (i64)(nx + 2) * (ny + 1), (double *)nullptr, (const double *)nullptr, (i64)0, 1.0 / p->dt);
        JRX_LAUNCH_CHECK(h);
    }
    PtLog log(res);
    int64_t iter = 0;
    const int rank = jrx_comm_rank(h);
    JRX_HIP(h, hipEventRecord(h->ev[6], s));
    auto keep_going = [&](int64_t it) { return it < 2 || ((log.rel() > p->eps_rel && log.err() > p->eps_abs) && it <= p->iterMax); };
    auto is_check = [&](int64_t i1) { return (i1 % p->nout == 0) && i1 > 1; };
    // Fused pipeline (as in 3D): when nothing observes iteration it1 and iteration it1+1 certainly runs unobserved, compute_V! of it1,
    // flow_bcs! (by rule) and the stress sweep of it1+1 run as one launch that ping-pongs (P, τ, V) between the caller's arrays and a
    // library-owned set; flow_bcs! itself is applied lazily before anything reads the boundary entries of V from memory.
    // measured with the XCD slab block order (SolCx, profiles/r02_bench2d_xcd_slabs.txt; it/s two kernels vs fused): 128^2 175.9 k / 176.2 k, 256^2 135.2 k /
    // 144.2 k, 384^2 101.5 k / 106.7 k, 512^2 79.1 k / 73.6 k, 768^2 40.1 k / 38.8 k, 1024^2 equal -- fused up to 200,000 nodes (~ 440^2)
    const bool fusable = !p->displacement_bcs && h->fused2d && h->scratch_sets && (h->kernel_variant == 3 || (h->kernel_variant == 0 && (i64)(nx + 1) * (ny + 1) <= (i64)(h->fused2d_batch ? h->fused2d_max_nodes : 200000))) &&
                         !jrx_comm_active(h) && p->periodic == 0 && nx >= 2 && ny >= 2 && !p->inv_spacing[0];
    const size_t nvx = (size_t)(nx + 1) * (ny + 2), nvy = (size_t)(nx + 2) * (ny + 1), nvt = (size_t)(nx + 1) * (ny + 1);
    Out6_2d setU = {f->P, f->txx, f->tyy, f->txy, f->Vx, f->Vy}, setS = setU;
    if (fusable) {
        if (!(h->scratch2d[0] && h->scratch2d_dims[0] == nx && h->scratch2d_dims[1] == ny)) {
            for (int q = 0; q < 6; q++) { if (h->scratch2d[q]) JRX_HIP(h, hipFree(h->scratch2d[q])); h->scratch2d[q] = nullptr; }
            h->scratch2d_dims[0] = h->scratch2d_dims[1] = 0;
            const size_t sz[6] = {n, n, n, nvt, nvx, nvy};
            for (int q = 0; q < 6; q++) JRX_HIP(h, hipMalloc(&h->scratch2d[q], sz[q] * sizeof(double)));
            h->scratch2d_dims[0] = nx; h->scratch2d_dims[1] = ny;
        }
        double **S = h->scratch2d;
        setS = Out6_2d{S[0], S[1], S[2], S[3], S[4], S[5]};
        // boundary and ghost entries of V that no fused launch writes
        JRX_HIP(h, hipMemcpyAsync(setS.Vx, f->Vx, nvx * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(setS.Vy, f->Vy, nvy * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    BC2 bc2;
    {
        auto ty = [&](uint32_t bit) { return (p->no_slip & bit) ? 2 : ((p->free_slip & bit) ? 1 : 0); };
        bc2.tL = ty(JRX_FACE_LEFT); bc2.tR = ty(JRX_FACE_RIGHT); bc2.tB = ty(JRX_FACE_BOT); bc2.tT = ty(JRX_FACE_TOP);
    }
    jrx_stokes2d_fields cur = *f;
    bool cur_is_user = true, stress_done = false, ghosts_stale = false;
    bool bcs_full_done[2] = {false, false};      // flow_bcs! launched in full on the V of the caller's set / the second set
    const int nwx = (nx + 1 + 62) / 63;
    // the one-launch iteration: "fused2d_batch" (default) = the form with every operand requested up front; its viscous-limit instantiation when dt = Inf and the operand check passed
    bool visc2 = false;
    if (fusable && h->fused2d_batch && h->viscous_limit && p->dt == INFINITY) {
        int *d_bad = reinterpret_cast<int *>(h->d_sums + 6), *h_bad = reinterpret_cast<int *>(h->h_sums + 6);
        JRX_HIP(h, hipMemsetAsync(d_bad, 0, sizeof(double), s));
        hipLaunchKernelGGL(k_visc_operands_ok2d, dim3(1024), dim3(256), 0, s, (const double *)f->P0, (const double *)f->Q, (const double *)f->toxx, (const double *)f->toyy,
                           (const double *)f->K, (const double *)f->G, (i64)n, (const double *)f->toxy, (i64)nvt, d_bad);
        JRX_LAUNCH_CHECK(h);
        JRX_HIP(h, hipMemcpyAsync(h_bad, d_bad, sizeof(double), hipMemcpyDeviceToHost, s));
        JRX_HIP(h, hipStreamSynchronize(s));
        visc2 = (*h_bad == 0);
        h->stat_visc_checks++;
        if (!visc2) h->stat_visc_fallbacks++;
    }
    const bool batch2 = h->fused2d_batch && (double)(nx + 2) * (double)(ny + 2) < 536870912.0;      // (32-bit byte offsets)
    auto launch_fused2d = [&](hipStream_t st, const Args2 &aa, const Out6_2d &dst) {
        const dim3 g((unsigned)((nwx * (ny + 1) + 3) / 4));
        if (batch2 && visc2) hipLaunchKernelGGL(k_fused2d_b<true>, g, dim3(256), 0, st, aa, dst, bc2, nwx);
        else if (batch2) hipLaunchKernelGGL(k_fused2d_b<false>, g, dim3(256), 0, st, aa, dst, bc2, nwx);
        else hipLaunchKernelGGL(k_fused2d, g, dim3(256), 0, st, aa, dst, bc2, nwx);
    };
    Args2 a = make_args2(&cur, h->etatau, p);
    // Runs of unobserved iterations in the steady state of the loop replay as a captured graph of GIT iterations (the gap between dependent launches is shorter
    // inside a graph: scripts/graph_probe.hip, 4.6 vs 5.7 - 6.1 us per pair of short kernels): GIT x k_fused2d (an even count, so that the ping-pong sets end where
    // they started; one graph per parity) on the grids that run the one-launch iteration (SolCx 128^2 173 k -> 184 k it/s, 256^2 143 k -> 150 k).  The two-kernel form
    // of the larger grids gains nothing from it (512^2: 77.9 k plain, 76.7 k replayed) and keeps plain launches.  Option "loop_graphs" = 0: plain launches everywhere.
    constexpr int GIT = 32;
    GraphExecs gexec;        // released on every exit path
    bool graphs = h->loop_graphs && fusable;
    // one fused step: the launch from the current set c into the other one, which becomes the current set
    auto fused_step = [&](jrx_stokes2d_fields &c, bool &c_is_user) {
        const Out6_2d dst = c_is_user ? setS : setU;
        launch_fused2d(s, make_args2(&c, h->etatau, p), dst);
        c.P = dst.P; c.txx = dst.txx; c.tyy = dst.tyy; c.txy = dst.txy; c.Vx = dst.Vx; c.Vy = dst.Vy;
        c_is_user = !c_is_user;
    };
    while (keep_going(iter)) {
        if (graphs && iter >= 2 && stress_done) {
            // observed iterations: the multiples of nout and iteration iterMax + 1 (Stokes2D.jl:265,312); between them err does not change, so keep_going holds.
            // The last unobserved iteration before an observed one is not fused with it: held back
            int64_t frun = pt_replay::unobserved_run(iter, p->nout, p->iterMax + 1, 1);
            if (frun >= GIT) {
                const int par = cur_is_user ? 0 : 1;
                if (!gexec[par]) {
                    JRX_TRY(jrx_capture_graph(s, &gexec[par], [&]() -> jrx_status {
                        jrx_stokes2d_fields c = cur;
                        bool cu = cur_is_user;
                        for (int q = 0; q < GIT; q++) fused_step(c, cu);
                        return JRX_OK;
                    }));
                    if (!gexec[par]) graphs = false;
                }
                if (gexec[par]) {
                    while (frun >= GIT) {
                        JRX_HIP(h, hipGraphLaunch(gexec[par], s));
                        iter += GIT; frun -= GIT;
                        h->stat_fused2d += GIT;
                        if (batch2) h->stat_fused2d_b += GIT;
                        h->stat_graph_replays++;
                    }
                    continue;
                }
            }
        }
        const int64_t it1 = iter + 1;
        const bool check = is_check(it1);
        const bool diag = check || !keep_going(it1);
        const bool fuse_next = fusable && !diag && keep_going(it1) && !(is_check(it1 + 1) || !keep_going(it1 + 1));
        a = make_args2(&cur, h->etatau, p);
        if (fuse_next) {
            if (!stress_done) {
                hipLaunchKernelGGL(k_stress2d<false>, dim3((unsigned)((nvt + 255) / 256)), dim3(256), 0, s, a);
                JRX_LAUNCH_CHECK(h);
            }
            fused_step(cur, cur_is_user);
            h->stat_fused2d++;
            if (batch2) h->stat_fused2d_b++;
            JRX_LAUNCH_CHECK(h);
            stress_done = true; ghosts_stale = true;
        } else {
            if (ghosts_stale && diag) {
                // U = V dt copies the boundary entries of V as flow_bcs! of the previous iteration left them: apply the pending flow_bcs! now
                JRX_TRY(jrx2d_bcs(h, s, cur.Vx, cur.Vy, nx, ny, p->free_slip, p->no_slip, p->periodic));
                bcs_full_done[cur_is_user ? 0 : 1] = true;
            }
            ghosts_stale = false;
            bool &full = bcs_full_done[cur_is_user ? 0 : 1];
            JRX_TRY(enqueue_iteration2(h, &cur, h->etatau, p, diag, full && iter >= 1, stress_done, &full));
            stress_done = false;
        }
        iter = it1;
        if (check) {
            a = make_args2(&cur, h->etatau, p);
            hipLaunchKernelGGL(k_velocity2d<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);   // compute_Res! (Stokes2D.jl:274-276)
            JRX_LAUNCH_CHECK(h);
            JRX_TRY(jrx2d_sumsq(h, s, f, p));
            double ss[4];
            JRX_TRY(jrx_read_sums(h, s, ss, true));
            const double nRx = sqrt(ss[0]) / sqrt((double)((p->nxg - 2) * (p->nyg - 1)));
            const double nRy = sqrt(ss[1]) / sqrt((double)((p->nxg - 1) * (p->nyg - 2)));
            const double nDV = sqrt(ss[3]) / sqrt((double)(p->nxg * p->nyg));      // jrx2d_sumsq leaves RP in slot 3
            const double err = log.record(iter, nRx, nRy, nDV);
            if (rank == 0 && ((p->verbose && log.rel() > p->eps_rel && err > p->eps_abs) || iter == p->iterMax)) log.print2d(iter, nRx, nRy, nDV);
        }
    }
    gexec.reset();
    JRX_HIP(h, hipEventRecord(h->ev[7], s));
    if (!cur_is_user) {       // leave the state in the caller's arrays
        JRX_HIP(h, hipMemcpyAsync(setU.P, setS.P, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(setU.txx, setS.txx, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(setU.tyy, setS.tyy, n * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(setU.txy, setS.txy, nvt * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(setU.Vx, setS.Vx, nvx * sizeof(double), hipMemcpyDeviceToDevice, s));
        JRX_HIP(h, hipMemcpyAsync(setU.Vy, setS.Vy, nvy * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    // multi_copy! (Stokes2D.jl:308-309)
    hipLaunchKernelGGL(k_copy6, dim3(256), dim3(256), 0, s, f->toxx, f->txx, (i64)n, f->toyy, f->tyy, (i64)n, f->toxy, f->txy, (i64)(nx + 1) * (ny + 1),
                       (f->txy_c && f->toxy_c) ? f->toxy_c : nullptr, (const double *)f->txy_c, (i64)n, (double *)nullptr, (const double *)nullptr,
                       (i64)0, (double *)nullptr, (const double *)nullptr, (i64)0);
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(s));
    float ms = 0.f;
    JRX_HIP(h, hipEventElapsedTime(&ms, h->ev[6], h->ev[7]));
    log.finish(iter, ms);
    return JRX_OK;
}

}   // extern "C"
