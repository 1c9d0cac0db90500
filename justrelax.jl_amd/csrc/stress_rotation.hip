// stress_rotation.hip -- grid-based rotation and advection of the old stress (rotate_stress!(stokes, grid, dt) on grids), for gfx950.
//
// Reference: the exported grid form rotate_stress!(V, τ, _di, dt), src/stress_rotation/stress_rotation_grid.jl.  That text is a stub and is NOT restated
// (include/jrx.h lists its defects); what is kept from the reference is the per-point rotation-matrix form rotate_stress_particles_rotation_matrix!
// (src/stress_rotation/stress_rotation_particles.jl:169-201, the products in the order of :182-197), the ω convention of compute_vorticity! (:17-80:
// ω_yz, ω_xz, ω_xy = half the curl's x, y, z component) and velocity2center (stress_rotation_grid.jl:171-176).
//
// One explicit, out-of-place step, both terms from the input state:   τ_o[c](I) = Rot_c(τ, ω dt)(I) - dt Adv(τ[c], v)(I)   at the member's own node I.
//
// A location is named by the set of axes along which it sits on a vertex (bit d = axis d): centre 0, the 2D vertex / 3D xy edge 3, the xz edge 5, the yz
// edge 6.  rs_interp<ND, T, S> brings an array that lives at location S to a node of location T: along an axis where the two differ the two nearest nodes
// of the source (target on a centre: I, I + 1; target on a vertex: I - 1, I clamped into the source's extent), the same node elsewhere; the 2^m values are
// summed in index order (x fastest) and multiplied by 1 / 2^m.  rs_vel does the same for a velocity component, whose ghost layers make every node exist
// (the centre j of a transverse axis is entry j + 1).  The rotation reads every quantity at the member's node; the upwind term is
// Σ_d v_d (v_d > 0 ? A[I] - A[I - e_d] : A[I + e_d] - A[I]) _d_d with a neighbour outside the array replaced by A[I].
//
// Shape (as phase_ratios.hip and k_vs3_stress): ONE launch, a thread per node of the ni .+ 1 box writes every member that has a node at its index -- in 2D
// the centre (xx, yy, xy_c) and the vertex (xy, optionally xx_v, yy_v), in 3D the centre (six members) and its yz, xz, xy edges.  Plain cached loads: the
// lanes of a wave and the rows of a block share almost every operand.  method and advection are template arguments.  No fma (the library builds with
// -ffp-contract=off): every product and sum is rounded once, in the order written, which is the order of tests/_stress_rotation.py.
// Addressing: 32-bit element offsets (every array below 2^31 entries, checked).
#include "op_args.hpp"
#include "rotate_point.hpp"

namespace {

constexpr int kRsTX = 64, kRsTY2 = 4;                 // 2D tile of nodes: 64 x 4
constexpr int kRsTY3 = 2, kRsTZ3 = 2;                 // 3D tile of nodes: 64 x 2 x 2

struct RsArgs {
    const double *t[9];        // inputs: 2D xx, yy, xy_c, xy, xx_v, yy_v; 3D xx, yy, zz, yz_c, xz_c, xy_c, yz, xz, xy
    double *o[9];              // outputs, same order
    const double *w[3];        // 2D: ω_xy in w[0]; 3D: ω_yz, ω_xz, ω_xy
    const double *v[3];        // Vx, Vy[, Vz] with their ghost layers (unread when ADV == 0)
    double idi[3];             // inverse spacings
    double dt;
    int n[3];                  // cells per axis (n[2] = 1 in 2D)
    int nbx, nby;              // blocks along x and y
};

// ------------------------------------------------------------------------------------------------ gathers
// the array A at location S (extents n .+ bits(S)) brought to the node I of location T
template <int ND, int T, int S>
__device__ __forceinline__ double rs_interp(const double *__restrict__ A, const int (&n)[3], const int (&I)[3])
{
    int idx[3][2], cnt[3], ext[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int td = (T >> d) & 1, sd = (S >> d) & 1;
        ext[d] = d < ND ? n[d] + sd : 1;
        if (d >= ND || td == sd) {
            cnt[d] = 1;
            idx[d][0] = idx[d][1] = d < ND ? I[d] : 0;
        } else if (td == 0) {            // centre from vertices: both exist
            cnt[d] = 2;
            idx[d][0] = I[d];
            idx[d][1] = I[d] + 1;
        } else {                         // vertex from centres: clamped into 0 .. n - 1
            cnt[d] = 2;
            idx[d][0] = I[d] - 1 < 0 ? 0 : I[d] - 1;
            idx[d][1] = I[d] > n[d] - 1 ? n[d] - 1 : I[d];
        }
    }
    double s = 0.0;
    bool first = true;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (c >= cnt[2]) continue;
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if (b >= cnt[1]) continue;
#pragma unroll
            for (int a = 0; a < 2; a++) {
                if (a >= cnt[0]) continue;
                const double x = A[(idx[2][c] * ext[1] + idx[1][b]) * ext[0] + idx[0][a]];
                s = first ? x : s + x;
                first = false;
            }
        }
    }
    return s * (1.0 / (double)(cnt[0] * cnt[1] * cnt[2]));
}

// velocity component C (vertices along C, centres with one ghost node either side along the other axes) brought to the node I of location T
template <int ND, int T, int C>
__device__ __forceinline__ double rs_vel(const double *__restrict__ A, const int (&n)[3], const int (&I)[3])
{
    int i0[3], cnt[3], ext[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int td = (T >> d) & 1;
        if (d >= ND) {
            ext[d] = 1, cnt[d] = 1, i0[d] = 0;
        } else if (d == C) {
            ext[d] = n[d] + 1, cnt[d] = td ? 1 : 2, i0[d] = I[d];
        } else {
            ext[d] = n[d] + 2, cnt[d] = td ? 2 : 1, i0[d] = td ? I[d] : I[d] + 1;
        }
    }
    double s = 0.0;
    bool first = true;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (c >= cnt[2]) continue;
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if (b >= cnt[1]) continue;
#pragma unroll
            for (int a = 0; a < 2; a++) {
                if (a >= cnt[0]) continue;
                const double x = A[((i0[2] + c) * ext[1] + i0[1] + b) * ext[0] + i0[0] + a];
                s = first ? x : s + x;
                first = false;
            }
        }
    }
    return s * (1.0 / (double)(cnt[0] * cnt[1] * cnt[2]));
}

template <int ND, int T>
__device__ __forceinline__ void rs_velocity(const RsArgs &a, const int (&I)[3], double (&v)[3])
{
    v[0] = rs_vel<ND, T, 0>(a.v[0], a.n, I);
    v[1] = rs_vel<ND, T, 1>(a.v[1], a.n, I);
    v[2] = ND == 3 ? rs_vel<ND, T, 2>(a.v[2], a.n, I) : 0.0;
}

// first-order upwind term of the array A at location S, at its own node I (value a0)
template <int ND, int S>
__device__ __forceinline__ double rs_upwind(const double *__restrict__ A, const RsArgs &a, const int (&I)[3], double a0, const double (&v)[3])
{
    const int ex = a.n[0] + (S & 1), ey = a.n[1] + ((S >> 1) & 1), ez = ND == 3 ? a.n[2] + ((S >> 2) & 1) : 1;
    const int ext[3] = {ex, ey, ez}, stride[3] = {1, ex, ex * ey};
    const int lin = (I[2] * ey + I[1]) * ex + I[0];
    double adv = 0.0;
#pragma unroll
    for (int d = 0; d < ND; d++) {
        const bool up = v[d] > 0.0;
        const bool inside = up ? I[d] > 0 : I[d] < ext[d] - 1;
        const double nb = A[inside ? (up ? lin - stride[d] : lin + stride[d]) : lin];          // outside: the node itself, an in-bounds load of a0
        const double term = v[d] * (up ? a0 - nb : nb - a0) * a.idi[d];
        adv = d == 0 ? term : adv + term;
    }
    return adv;
}

// ------------------------------------------------------------------------------------------------ rotations
// rs_rot2<METHOD>, the per-point 2D rotation: rotate_point.hpp (shared with particles.hip)

// t, o: xx, yy, zz, yz, xz, xy; w: ω_yz, ω_xz, ω_xy (the axial vector).  METHOD 0: Rodrigues, θ = dt |w|, n = w / |w| (|w| == 0: n = 0, R = I, no division);
// METHOD 1: τ + (A τ - τ A) with A = [dt w]x
template <int METHOD>
__device__ __forceinline__ void rs_rot3(const double (&t)[6], const double (&w)[3], double dt, double (&o)[6])
{
    const double T[3][3] = {{t[0], t[5], t[4]}, {t[5], t[1], t[3]}, {t[4], t[3], t[2]}};
    double O[3][3];
    if (METHOD == 0) {
        const double nrm = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
        const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
        const double nx = w[0] * inv, ny = w[1] * inv, nz = w[2] * inv;
        double s, c;
        sincos(dt * nrm, &s, &c);
        const double c1 = 1.0 - c;
        const double xy = nx * ny, xz = nx * nz, yz = ny * nz;
        const double R[3][3] = {{1.0 + c1 * -(ny * ny + nz * nz), s * -nz + c1 * xy, s * ny + c1 * xz},
                                {s * nz + c1 * xy, 1.0 + c1 * -(nx * nx + nz * nz), s * -nx + c1 * yz},
                                {s * -ny + c1 * xz, s * nx + c1 * yz, 1.0 + c1 * -(nx * nx + ny * ny)}};
        double M[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) M[i][j] = (T[i][0] * R[j][0] + T[i][1] * R[j][1]) + T[i][2] * R[j][2];      // τ R'
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) O[i][j] = (R[i][0] * M[0][j] + R[i][1] * M[1][j]) + R[i][2] * M[2][j];      // R (τ R')
    } else {
        const double ax = dt * w[0], ay = dt * w[1], az = dt * w[2];
        const double A[3][3] = {{0.0, -az, ay}, {az, 0.0, -ax}, {-ay, ax, 0.0}};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) {
                const int k1 = (i + 1) % 3, k2 = (i + 2) % 3, l1 = (j + 1) % 3, l2 = (j + 2) % 3;      // the entries of row i of A / column j of A that are not 0
                const double p = A[i][k1] * T[k1][j] + A[i][k2] * T[k2][j];                            // (A τ)_ij
                const double q = T[i][l1] * A[l1][j] + T[i][l2] * A[l2][j];                            // (τ A)_ij
                O[i][j] = T[i][j] + (p - q);
            }
    }
    o[0] = O[0][0], o[1] = O[1][1], o[2] = O[2][2], o[3] = O[1][2], o[4] = O[0][2], o[5] = O[0][1];
}

// ------------------------------------------------------------------------------------------------ kernels
template <int ND>
__device__ __forceinline__ void rs_index(int nbx, int nby, int (&I)[3])
{
    int b = (int)blockIdx.x;
    const int bx = b % nbx;
    b /= nbx;
    I[0] = bx * kRsTX + (int)threadIdx.x;
    if (ND == 2) {
        I[1] = b * kRsTY2 + (int)threadIdx.y;
        I[2] = 0;
    } else {
        I[1] = (b % nby) * kRsTY3 + (int)threadIdx.y;
        I[2] = (b / nby) * kRsTZ3 + (int)threadIdx.z;
    }
}

// VTXN: the optional vertex normals xx_v, yy_v are present
template <int METHOD, int ADV, int VTXN>
__global__ __launch_bounds__(256) void k_rotate_stress2d(const RsArgs a)
{
    int I[3];
    rs_index<2>(a.nbx, a.nby, I);
    const int nx = a.n[0], ny = a.n[1];
    if (I[0] > nx || I[1] > ny) return;
    double v[3] = {0.0, 0.0, 0.0};
    if (I[0] < nx && I[1] < ny) {                                  // centre: xx, yy, xy_c from their own node, ω from the four vertices
        const int lin = I[1] * nx + I[0];
        const double xx = a.t[0][lin], yy = a.t[1][lin], xy = a.t[2][lin];
        const double th = a.dt * rs_interp<2, 0, 3>(a.w[0], a.n, I);
        double r[3];
        rs_rot2<METHOD>(xx, yy, xy, th, r[0], r[1], r[2]);
        if (ADV) {
            rs_velocity<2, 0>(a, I, v);
            r[0] -= a.dt * rs_upwind<2, 0>(a.t[0], a, I, xx, v);
            r[1] -= a.dt * rs_upwind<2, 0>(a.t[1], a, I, yy, v);
            r[2] -= a.dt * rs_upwind<2, 0>(a.t[2], a, I, xy, v);
        }
        a.o[0][lin] = r[0], a.o[1][lin] = r[1], a.o[2][lin] = r[2];
    }
    {                                                              // vertex: xy with the normals from the four centres; xx_v, yy_v from their own node
        const int lin = I[1] * (nx + 1) + I[0];
        const double xy = a.t[3][lin];
        const double th = a.dt * a.w[0][lin];
        const double xx = rs_interp<2, 3, 0>(a.t[0], a.n, I), yy = rs_interp<2, 3, 0>(a.t[1], a.n, I);
        double r[3], q[3] = {0.0, 0.0, 0.0}, xxv = 0.0, yyv = 0.0;
        rs_rot2<METHOD>(xx, yy, xy, th, r[0], r[1], r[2]);
        if (VTXN) {
            xxv = a.t[4][lin], yyv = a.t[5][lin];
            rs_rot2<METHOD>(xxv, yyv, xy, th, q[0], q[1], q[2]);
        }
        if (ADV) {
            rs_velocity<2, 3>(a, I, v);
            r[2] -= a.dt * rs_upwind<2, 3>(a.t[3], a, I, xy, v);
            if (VTXN) {
                q[0] -= a.dt * rs_upwind<2, 3>(a.t[4], a, I, xxv, v);
                q[1] -= a.dt * rs_upwind<2, 3>(a.t[5], a, I, yyv, v);
            }
        }
        a.o[3][lin] = r[2];
        if (VTXN) a.o[4][lin] = q[0], a.o[5][lin] = q[1];
    }
}

// the edge member at location S (6 = yz, 5 = xz, 3 = xy; arrays 6, 7, 8 and Voigt components 3, 4, 5) of the node I
template <int METHOD, int ADV, int S>
__device__ __forceinline__ void rs_edge3(const RsArgs &a, const int (&I)[3])
{
    constexpr int M = S == 6 ? 6 : (S == 5 ? 7 : 8), C = M - 3;
    const int ex = a.n[0] + (S & 1), ey = a.n[1] + ((S >> 1) & 1);
    const int lin = (I[2] * ey + I[1]) * ex + I[0];
    const double own = a.t[M][lin];
    double t[6], w[3], o[6];
    t[0] = rs_interp<3, S, 0>(a.t[0], a.n, I);
    t[1] = rs_interp<3, S, 0>(a.t[1], a.n, I);
    t[2] = rs_interp<3, S, 0>(a.t[2], a.n, I);
    t[3] = S == 6 ? own : rs_interp<3, S, 6>(a.t[6], a.n, I);
    t[4] = S == 5 ? own : rs_interp<3, S, 5>(a.t[7], a.n, I);
    t[5] = S == 3 ? own : rs_interp<3, S, 3>(a.t[8], a.n, I);
    w[0] = rs_interp<3, S, 6>(a.w[0], a.n, I);
    w[1] = rs_interp<3, S, 5>(a.w[1], a.n, I);
    w[2] = rs_interp<3, S, 3>(a.w[2], a.n, I);
    rs_rot3<METHOD>(t, w, a.dt, o);
    double r = o[C];
    if (ADV) {
        double v[3];
        rs_velocity<3, S>(a, I, v);
        r -= a.dt * rs_upwind<3, S>(a.t[M], a, I, own, v);
    }
    a.o[M][lin] = r;
}

template <int METHOD, int ADV>
__global__ __launch_bounds__(256) void k_rotate_stress3d(const RsArgs a)
{
    int I[3];
    rs_index<3>(a.nbx, a.nby, I);
    const int nx = a.n[0], ny = a.n[1], nz = a.n[2];
    if (I[0] > nx || I[1] > ny || I[2] > nz) return;
    const bool ix = I[0] < nx, iy = I[1] < ny, iz = I[2] < nz;
    if (ix && iy && iz) {                                          // centre: six members from their own node, ω from the four edges of each family
        const int lin = (I[2] * ny + I[1]) * nx + I[0];
        double t[6], w[3], o[6];
#pragma unroll
        for (int c = 0; c < 6; c++) t[c] = a.t[c][lin];
        w[0] = rs_interp<3, 0, 6>(a.w[0], a.n, I);
        w[1] = rs_interp<3, 0, 5>(a.w[1], a.n, I);
        w[2] = rs_interp<3, 0, 3>(a.w[2], a.n, I);
        rs_rot3<METHOD>(t, w, a.dt, o);
        if (ADV) {
            double v[3];
            rs_velocity<3, 0>(a, I, v);
#pragma unroll
            for (int c = 0; c < 6; c++) o[c] -= a.dt * rs_upwind<3, 0>(a.t[c], a, I, t[c], v);
        }
#pragma unroll
        for (int c = 0; c < 6; c++) a.o[c][lin] = o[c];
    }
    if (ix) rs_edge3<METHOD, ADV, 6>(a, I);
    if (iy) rs_edge3<METHOD, ADV, 5>(a, I);
    if (iz) rs_edge3<METHOD, ADV, 3>(a, I);
}

// ------------------------------------------------------------------------------------------------ host
// checks and launch shared by the two entry points.  tau / tau_o: NT members with the staggering sets stag[]; the first `req` are required
jrx_status rs_rotate(jrx_handle *h, const char *fn, int ND, double *const *tau_o, const double *const *tau, const char *const *names, const int *stag, int NT, int req,
                     const double *const *omega, const char *const *wnames, const int *wstag, int NW, const double *const *V, const int64_t n[3], const double *_di,
                     double dt, int32_t method, int32_t advection)
{
    if (!h) return JRX_ERR_ARG;
    if (!tau_o || !tau || !omega || !_di) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    if (method != JRX_ROTATE_MATRIX && method != JRX_ROTATE_JAUMANN)
        return jrx_fail(h, JRX_ERR_ARG, "%s: unknown method %d (%d = matrix, %d = jaumann)", fn, (int)method, JRX_ROTATE_MATRIX, JRX_ROTATE_JAUMANN);
    if (advection != JRX_ADVECT_NONE && advection != JRX_ADVECT_UPWIND)
        return jrx_fail(h, JRX_ERR_ARG, "%s: unknown advection kind %d (%d = none, %d = upwind)", fn, (int)advection, JRX_ADVECT_NONE, JRX_ADVECT_UPWIND);
    for (int d = 0; d < ND; d++)
        if (n[d] < 1) return jrx_fail(h, JRX_ERR_ARG, "%s: extent %lld along dimension %d", fn, (long long)n[d], d + 1);
    // a box that holds every array: the velocities have n + 2 along their transverse axes
    if (op_2g(op_count(n, ND, 2))) return jrx_fail(h, JRX_ERR_ARG, "%s: the velocity box (ni .+ 2) has 2^31 or more entries (32-bit offsets)", fn);
    const bool adv = advection == JRX_ADVECT_UPWIND;
    if (adv && !V) return jrx_fail(h, JRX_ERR_ARG, "%s: V is NULL (only advection = none takes no velocities)", fn);
    auto at = [&](int S) { return op_bytes(n, ND, S & 1, (S >> 1) & 1, (S >> 2) & 1); };       // bytes of an array at location S
    bool present[9] = {};
    const bool opt = NT > req && tau[req] && tau[req + 1] && tau_o[req] && tau_o[req + 1];       // the 2D vertex normals: all four or none
    OpArr in[16], out[9];
    int nin = 0, nout = 0;
    for (int m = 0; m < NT; m++) {
        if (m >= req) {
            present[m] = opt;
            if (!opt) continue;
        } else {
            if (!tau[m]) return jrx_fail(h, JRX_ERR_ARG, "%s: τ.%s is NULL", fn, names[m]);
            if (!tau_o[m]) return jrx_fail(h, JRX_ERR_ARG, "%s: τ_o.%s is NULL", fn, names[m]);
            present[m] = true;
        }
        in[nin++] = {tau[m], at(stag[m]), names[m]};
        out[nout++] = {tau_o[m], at(stag[m]), names[m]};
    }
    static const char *const vnames[3] = {"V.Vx", "V.Vy", "V.Vz"};
    for (int c = 0; c < NW; c++) {
        if (!omega[c]) return jrx_fail(h, JRX_ERR_ARG, "%s: ω.%s is NULL", fn, wnames[c]);
        in[nin++] = {omega[c], at(wstag[c]), wnames[c]};
    }
    if (adv)
        for (int c = 0; c < ND; c++) {
            if (!V[c]) return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL (only advection = none takes no velocities)", fn, vnames[c]);
            in[nin++] = {V[c], op_vel_bytes(n, ND, c), vnames[c]};
        }
    if (const OpClash c = op_disjoint(out, nout, in, nin))
        return c.two ? jrx_fail(h, JRX_ERR_ARG, "%s: outputs τ_o.%s and τ_o.%s overlap", fn, out[c.a].name, out[c.b].name)
                     : jrx_fail(h, JRX_ERR_ARG, "%s: output τ_o.%s overlaps input %s (the step is out of place)", fn, out[c.a].name, in[c.b].name);
    JRX_TRY(jrx_check_device(h));
    RsArgs a = {};
    for (int m = 0; m < NT; m++)
        if (present[m]) a.t[m] = tau[m], a.o[m] = tau_o[m];
    for (int c = 0; c < NW; c++) a.w[c] = omega[c];
    a.n[2] = 1;
    for (int d = 0; d < ND; d++) {
        if (adv) a.v[d] = V[d];
        a.idi[d] = _di[d];
        a.n[d] = (int)n[d];
    }
    a.dt = dt;
    const int ty = ND == 2 ? kRsTY2 : kRsTY3, tz = ND == 2 ? 1 : kRsTZ3;
    a.nbx = (a.n[0] + 1 + kRsTX - 1) / kRsTX;
    a.nby = (a.n[1] + 1 + ty - 1) / ty;
    const int64_t nb = (int64_t)a.nbx * a.nby * (ND == 3 ? (a.n[2] + 1 + tz - 1) / tz : 1);      // below 2^31: the box is below 2^31 entries
    h->stat_rotate_stress_calls++;
    dispatch_const<0, 1>((int)method, [&](auto MM) {
        dispatch_const<0, 1>(adv ? 1 : 0, [&](auto AA) {
            constexpr int M = MM(), A = AA();
            if (ND == 3) hipLaunchKernelGGL((k_rotate_stress3d<M, A>), dim3((unsigned)nb), dim3(kRsTX, ty, tz), 0, h->stream, a);
            else if (opt) hipLaunchKernelGGL((k_rotate_stress2d<M, A, 1>), dim3((unsigned)nb), dim3(kRsTX, ty, tz), 0, h->stream, a);
            else hipLaunchKernelGGL((k_rotate_stress2d<M, A, 0>), dim3((unsigned)nb), dim3(kRsTX, ty, tz), 0, h->stream, a);
        });
    });
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_rotate_stress2d(jrx_handle *h, double *const tau_o[6], const double *const tau[6], const double *omega_xy, const double *const V[2], int64_t nx,
                               int64_t ny, const double _di[2], double dt, int32_t method, int32_t advection)
{
    static const char *const names[6] = {"xx", "yy", "xy_c", "xy", "xx_v", "yy_v"};
    static const int stag[6] = {0, 0, 0, 3, 3, 3};
    static const char *const wnames[1] = {"xy"};
    static const int wstag[1] = {3};
    const double *const omega[1] = {omega_xy};
    const int64_t n[3] = {nx, ny, 1};
    return rs_rotate(h, "rotate_stress! (2D)", 2, tau_o, tau, names, stag, 6, 4, omega, wnames, wstag, 1, V, n, _di, dt, method, advection);
}

jrx_status jrx_rotate_stress3d(jrx_handle *h, double *const tau_o[9], const double *const tau[9], const double *const omega[3], const double *const V[3],
                               int64_t nx, int64_t ny, int64_t nz, const double _di[3], double dt, int32_t method, int32_t advection)
{
    static const char *const names[9] = {"xx", "yy", "zz", "yz_c", "xz_c", "xy_c", "yz", "xz", "xy"};
    static const int stag[9] = {0, 0, 0, 0, 0, 0, 6, 5, 3};
    static const char *const wnames[3] = {"yz", "xz", "xy"};
    static const int wstag[3] = {6, 5, 3};
    const int64_t n[3] = {nx, ny, nz};
    return rs_rotate(h, "rotate_stress! (3D)", 3, tau_o, tau, names, stag, 9, 9, omega, wnames, wstag, 3, V, n, _di, dt, method, advection);
}

}  // extern "C"
