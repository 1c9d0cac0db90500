// phase_ratios.hip -- phase ratios from N advected phase fields (update_phase_ratios_2D! / update_phase_ratios_3D!), for gfx950.
//
// Reference being replaced (PTsolvers/JustRelax.jl): src/phases/PhaseRatios.jl:24-35 (2D driver: four launches), :61-78 (3D driver: eight launches),
// :89-116 (centres), :135-211 (vertices: bilinear weights through muladd in 2D, the trilinear product without it in 3D), :231-293 (faces), :324-383 (edges).
// Inputs are N cell-centred arrays p_1..p_N of (nx, ny[, nz]) entries; outputs are the members of a PhaseRatios in CellArray layout (phase index fastest).
//
// Every member of a node is built from the same 2^ndim cells at offsets {-1, 0} per dimension.  Cell c of that neighbourhood has the x offset in its
// highest bit and the last dimension's in its lowest (bit set = offset 0), so c = 0 .. 2^ndim - 1 IS the reference's visiting order (first dimension
// outermost, -1 before 0).  A member is named by the set S of dimensions it is staggered in (bit d = dimension d): centre 0, Vx 1, Vy 2, xy 3, Vz 4, xz 5,
// yz 6, and the vertex all of them (3 in 2D, 7 in 3D).  Member S reads the cells whose offset is 0 in every dimension outside S, in ascending c -- which
// is the order the reference's face loop (side = 0, 1) and edge loop (corner = 1..4) visit them in -- skips the ones outside the grid, and applies one
// common tail: divide by the accumulated weight (centres: by the sum of the values), clamp to [0, 1] by comparisons (a NaN stays a NaN, as Julia's clamp
// and min(max()) leave it), values < 1e-5 become 0, divide by the sum of what is left.  Every sum runs over the phases left to right.
// The accumulated weight of a face or an edge is 0.5 or 1 (0.25, 0.5 or 1): dividing by it is written as the product with its reciprocal, which gives the
// same bits (both are exact scalings by a power of two).  The vertex weight is an arbitrary double and is divided by.
//
// Two forms built from the same __device__ function pr_node, so every member comes out bit-identical:
//   fused (default, tuning "phase_ratios_fused" = 1): ONE launch, one thread per node of the (ni .+ 1) box.  The thread loads the 2^ndim x N values around
//     its node once, with plain cached loads (the x - 1 neighbour of a lane is the lane beside it and the y - 1 / z - 1 rows belong to the same or the
//     neighbouring block: they hit in L1 / L2; no LDS tile, no barrier), and writes every member that has a node at its index.  N is a template argument
//     (1 .. JRX_MAXPHASE), so the values live in registers; a thread stores N contiguous doubles per member and a wave's stores are contiguous.
//   per member ("phase_ratios_fused" = 0): the reference's shape, one launch per member over that member's extents (4 in 2D, 8 in 3D); a launch loads only
//     the cells its member reads.
// fma() stands where the reference has muladd (the 2D vertex weights); the library builds with -ffp-contract=off, so nothing else is contracted.
// Addressing: 32-bit element offsets (every output below 2^31 entries, checked).
#include "op_args.hpp"

namespace {

constexpr int kPrTX = 64, kPrTY2 = 4;                 // 2D tile of nodes: 64 x 4
constexpr int kPrTY3 = 2, kPrTZ3 = 2;                 // 3D tile of nodes: 64 x 2 x 2

template <int N>
struct PrArgs {
    const double *p[N];        // phase arrays
    double *out[8];            // members by staggering set S (see above); unused entries NULL
    const double *xc[3], *xv[3];
    double idx[3];             // inv(dx_d)
    int n[3];                  // cells per dimension (n[2] = 1 in 2D)
    int nbx, nby;              // blocks along x and y of the launch
};

constexpr int pr_bit(int ND, int d) { return ND - 1 - d; }                     // bit of cell c that holds dimension d's offset
constexpr bool pr_uses(int ND, int S, int c)                                    // member S reads cell c
{
    for (int d = 0; d < ND; d++)
        if (!((S >> d) & 1) && !((c >> pr_bit(ND, d)) & 1)) return false;
    return true;
}
constexpr bool pr_needed(int ND, int MS, int c)                                 // some member of the set MS (bit S = member S) reads cell c
{
    for (int S = 0; S < (1 << ND); S++)
        if (((MS >> S) & 1) && pr_uses(ND, S, c)) return true;
    return false;
}
constexpr int pr_popcount(int S) { return (S & 1) + ((S >> 1) & 1) + ((S >> 2) & 1); }

// the common tail (PhaseRatios.jl:100-113, :193-208, :271-290, :361-380) on values already divided by their weight
template <int N>
__device__ __forceinline__ void pr_tail(double (&w)[N], double *__restrict__ out)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double x = w[k];
        x = x > 1.0 ? 1.0 : (x < 0.0 ? 0.0 : x);
        x = x < 1.0e-5 ? 0.0 : x;
        w[k] = x;
        s += x;
    }
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = w[k] / s;
}

// the members MS of the node I (0-based) whose staggered extents contain it
template <int N, int ND, int MS>
__device__ __forceinline__ void pr_node(const PrArgs<N> &a, const int (&I)[3])
{
    constexpr int NC = 1 << ND, VTX = NC - 1;
    bool lo[3], hi[3];                      // the cell at offset -1 / 0 along d is inside the grid
#pragma unroll
    for (int d = 0; d < ND; d++) {
        lo[d] = I[d] >= 1;
        hi[d] = I[d] < a.n[d];
    }
    double p[NC][N];
    bool ok[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (!pr_needed(ND, MS, c)) continue;
        bool v = true;
        int off = 0;
#pragma unroll
        for (int d = ND - 1; d >= 0; d--) {
            const bool o0 = (c >> pr_bit(ND, d)) & 1;
            v = v && (o0 ? hi[d] : lo[d]);
            off = off * a.n[d] + (o0 ? I[d] : I[d] - 1);
        }
        ok[c] = v;
#pragma unroll
        for (int k = 0; k < N; k++) p[c][k] = v ? a.p[k][off] : 0.0;
    }
    // vertex weights (PhaseRatios.jl:150-155 with muladd, :171-178 without)
    double f[3][2];
    if constexpr ((MS >> VTX) & 1) {
#pragma unroll
        for (int d = 0; d < ND; d++) {
            const double xv = a.xv[d][I[d]];
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const bool v = o ? hi[d] : lo[d];
                const double xc = a.xc[d][v ? I[d] - 1 + o : 0];
                const double dist = fabs(xv - xc);
                f[d][o] = ND == 2 ? fma(-dist, a.idx[d], 1.0) : 1.0 - dist * a.idx[d];
            }
        }
    }
#pragma unroll
    for (int S = 0; S < NC; S++) {
        if (!((MS >> S) & 1)) continue;
        bool inside = true;
        int lin = 0;
#pragma unroll
        for (int d = ND - 1; d >= 0; d--) {
            const bool st = (S >> d) & 1;
            inside = inside && (st || hi[d]);
            lin = lin * (a.n[d] + (st ? 1 : 0)) + I[d];
        }
        if (!inside) continue;
        double w[N];
        if (S == 0) {                       // centres: values ./ sum(values)
            double t = p[VTX][0];
#pragma unroll
            for (int k = 1; k < N; k++) t += p[VTX][k];
#pragma unroll
            for (int k = 0; k < N; k++) w[k] = p[VTX][k] / t;
        } else {
            double W = 0.0;
#pragma unroll
            for (int k = 0; k < N; k++) w[k] = 0.0;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (!pr_uses(ND, S, c)) continue;
                double wt;
                if (S == VTX) {
                    wt = f[0][(c >> pr_bit(ND, 0)) & 1] * f[1][(c >> pr_bit(ND, 1)) & 1];
                    if (ND == 3) wt *= f[2][c & 1];
                } else {
                    wt = pr_popcount(S) == 1 ? 0.5 : 0.25;
                }
                if (ok[c]) {
                    W += wt;
#pragma unroll
                    for (int k = 0; k < N; k++) w[k] += wt * p[c][k];
                }
            }
            if (S == VTX) {
#pragma unroll
                for (int k = 0; k < N; k++) w[k] /= W;
            } else {                        // W is 0.25, 0.5 or 1: the product with 1 / W has the quotient's bits
                const double rW = 1.0 / W;
#pragma unroll
                for (int k = 0; k < N; k++) w[k] *= rW;
            }
        }
        pr_tail<N>(w, a.out[S] + (size_t)lin * N);
    }
}

// block -> tile of nodes; false for a thread outside the box of the member set's largest extents (n[d] + 1 where some member of the launch is staggered)
template <int ND>
__device__ __forceinline__ void pr_index(int nbx, int nby, int (&I)[3])
{
    int b = (int)blockIdx.x;
    const int bx = b % nbx;
    b /= nbx;
    I[0] = bx * kPrTX + (int)threadIdx.x;
    if (ND == 2) {
        I[1] = b * kPrTY2 + (int)threadIdx.y;
        I[2] = 0;
    } else {
        I[1] = (b % nby) * kPrTY3 + (int)threadIdx.y;
        I[2] = (b / nby) * kPrTZ3 + (int)threadIdx.z;
    }
}

// fused form: every member, one thread per node of the (ni .+ 1) box
template <int N, int ND>
__global__ __launch_bounds__(256) void k_phase_ratios(const PrArgs<N> a)
{
    int I[3];
    pr_index<ND>(a.nbx, a.nby, I);
    for (int d = 0; d < ND; d++)
        if (I[d] > a.n[d]) return;
    pr_node<N, ND, (1 << (1 << ND)) - 1>(a, I);
}

// per-member form: member S over its own extents
template <int N, int ND, int S>
__global__ __launch_bounds__(256) void k_phase_ratios_member(const PrArgs<N> a)
{
    int I[3];
    pr_index<ND>(a.nbx, a.nby, I);
    for (int d = 0; d < ND; d++)
        if (I[d] >= a.n[d] + ((S >> d) & 1)) return;
    pr_node<N, ND, 1 << S>(a, I);
}

template <int N, int ND>
void pr_launch_box(jrx_handle *h, PrArgs<N> a, int S, void (*kern)(const PrArgs<N>))
{
    const int ex = a.n[0] + (S & 1), ey = a.n[1] + ((S >> 1) & 1), ez = ND == 3 ? a.n[2] + ((S >> 2) & 1) : 1;
    const int ty = ND == 2 ? kPrTY2 : kPrTY3, tz = ND == 2 ? 1 : kPrTZ3;
    a.nbx = (ex + kPrTX - 1) / kPrTX;
    a.nby = (ey + ty - 1) / ty;
    const int64_t nb = (int64_t)a.nbx * a.nby * ((ez + tz - 1) / tz);      // below 2^31: every output is below 2^31 entries
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(kPrTX, ty, tz), 0, h->stream, a);
}

template <int N, int ND>
void pr_launch(jrx_handle *h, const PrArgs<N> &a, bool fused)
{
    constexpr int VTX = (1 << ND) - 1;
    if (fused) {
        pr_launch_box<N, ND>(h, a, VTX, k_phase_ratios<N, ND>);
        return;
    }
    // the reference's order: centres, vertices, faces, then (3D) xy, yz, xz
    pr_launch_box<N, ND>(h, a, 0, k_phase_ratios_member<N, ND, 0>);
    pr_launch_box<N, ND>(h, a, VTX, k_phase_ratios_member<N, ND, VTX>);
    pr_launch_box<N, ND>(h, a, 1, k_phase_ratios_member<N, ND, 1>);
    pr_launch_box<N, ND>(h, a, 2, k_phase_ratios_member<N, ND, 2>);
    if constexpr (ND == 3) {
        pr_launch_box<N, ND>(h, a, 4, k_phase_ratios_member<N, ND, 4>);
        pr_launch_box<N, ND>(h, a, 3, k_phase_ratios_member<N, ND, 3>);
        pr_launch_box<N, ND>(h, a, 6, k_phase_ratios_member<N, ND, 6>);
        pr_launch_box<N, ND>(h, a, 5, k_phase_ratios_member<N, ND, 5>);
    }
}

// checks and launch shared by the two entry points; out / names by staggering set S, NULL where ndim has no such member
jrx_status pr_update(jrx_handle *h, const char *fn, int ND, double *const out[8], const char *const names[8], const double *const *phase_arrays, int32_t nphase,
                     const int64_t n[3], const double *const *xc, const double *const *xv, const double *dx)
{
    if (!h) return JRX_ERR_ARG;
    const int NC = 1 << ND;
    if (!phase_arrays || !xc || !xv || !dx) return jrx_fail(h, JRX_ERR_ARG, "%s: NULL argument", fn);
    OpArr o[8], in[JRX_MAXPHASE + 6];            // inputs: the phase arrays, then xc and xv of each dimension
    for (int S = 0; S < NC; S++) o[S] = OpArr{out[S], 0, names[S]};
    JRX_TRY(op_present(h, fn, o, NC));
    if (nphase < 1 || nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phase arrays (1 .. %d are built)", fn, (int)nphase, JRX_MAXPHASE);
    for (int k = 0; k < nphase; k++)
        if (!phase_arrays[k]) return jrx_fail(h, JRX_ERR_ARG, "%s: phase array %d is NULL", fn, k + 1);
    for (int d = 0; d < ND; d++) {
        if (!xc[d] || !xv[d]) return jrx_fail(h, JRX_ERR_ARG, "%s: coordinate vector of dimension %d is NULL", fn, d + 1);
        if (n[d] < 1) return jrx_fail(h, JRX_ERR_ARG, "%s: extent %lld along dimension %d", fn, (long long)n[d], d + 1);
        if (!op_pos_finite(dx[d])) return jrx_fail(h, JRX_ERR_ARG, "%s: spacing %g along dimension %d (must be positive and finite)", fn, dx[d], d + 1);
    }
    // the largest output is the vertex array
    if (op_2g((double)nphase * op_count(n, ND, 1))) return jrx_fail(h, JRX_ERR_UNSUPPORTED, "%s: phase_ratios.vertex has 2^31 or more entries (32-bit offsets)", fn);
    for (int S = 0; S < NC; S++) o[S].bytes = nphase * op_bytes(n, ND, S & 1, (S >> 1) & 1, (S >> 2) & 1);
    for (int k = 0; k < nphase; k++) in[k] = OpArr{phase_arrays[k], op_bytes(n, ND, 0, 0, 0), nullptr};
    for (int d = 0; d < ND; d++) in[nphase + 2 * d] = OpArr{xc[d], 8 * n[d], nullptr}, in[nphase + 2 * d + 1] = OpArr{xv[d], 8 * (n[d] + 1), nullptr};
    if (const OpClash c = op_disjoint(o, NC, in, nphase + 2 * ND)) {
        if (c.two) return jrx_fail(h, JRX_ERR_ARG, "%s: %s and %s overlap", fn, o[c.a].name, o[c.b].name);
        return c.b < nphase ? jrx_fail(h, JRX_ERR_ARG, "%s: %s overlaps phase array %d", fn, o[c.a].name, c.b + 1)
                            : jrx_fail(h, JRX_ERR_ARG, "%s: %s overlaps a coordinate vector of dimension %d", fn, o[c.a].name, (c.b - nphase) / 2 + 1);
    }
    JRX_TRY(jrx_check_device(h));
    const bool fused = h->phase_ratios_fused;
    h->stat_phase_ratios_calls++;
    if (fused) h->stat_phase_ratios_fused++;
    dispatch_const<1, 2, 3, 4, 5, 6, 7, 8>((int)nphase, [&](auto NP) {
        constexpr int N = NP();
        PrArgs<N> a = {};
        for (int k = 0; k < N; k++) a.p[k] = phase_arrays[k];
        for (int S = 0; S < NC; S++) a.out[S] = out[S];
        a.n[2] = 1;
        for (int d = 0; d < ND; d++) {
            a.xc[d] = xc[d];
            a.xv[d] = xv[d];
            a.idx[d] = 1.0 / dx[d];              // inv(dx)
            a.n[d] = (int)n[d];
        }
        if (ND == 2) pr_launch<N, 2>(h, a, fused);
        else pr_launch<N, 3>(h, a, fused);
    });
    return op_finish(h);
}

}  // namespace

extern "C" {

jrx_status jrx_update_phase_ratios2d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *const *phase_arrays, int32_t nphase,
                                     int64_t nx, int64_t ny, const double *const xc[2], const double *const xv[2], const double dx[2])
{
    double *const out[8] = {center, Vx, Vy, vertex, nullptr, nullptr, nullptr, nullptr};
    const char *const names[8] = {"phase_ratios.center", "phase_ratios.Vx", "phase_ratios.Vy", "phase_ratios.vertex", "", "", "", ""};
    const int64_t n[3] = {nx, ny, 1};
    return pr_update(h, "update_phase_ratios_2D!", 2, out, names, phase_arrays, nphase, n, xc, xv, dx);
}

jrx_status jrx_update_phase_ratios3d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, double *Vz, double *yz, double *xz, double *xy,
                                     const double *const *phase_arrays, int32_t nphase, int64_t nx, int64_t ny, int64_t nz, const double *const xc[3],
                                     const double *const xv[3], const double dx[3])
{
    double *const out[8] = {center, Vx, Vy, xy, Vz, xz, yz, vertex};
    const char *const names[8] = {"phase_ratios.center", "phase_ratios.Vx", "phase_ratios.Vy", "phase_ratios.xy",
                                  "phase_ratios.Vz",     "phase_ratios.xz", "phase_ratios.yz", "phase_ratios.vertex"};
    const int64_t n[3] = {nx, ny, nz};
    return pr_update(h, "update_phase_ratios_3D!", 3, out, names, phase_arrays, nphase, n, xc, xv, dx);
}

}  // extern "C"
