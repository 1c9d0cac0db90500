// particles_common.hpp -- what the 2D (particles.hip) and the 3D (particles3d.hip) particle operators share.  Device side: the per-axis pieces of every definition
// of include/jrx.h (the finite test, the clamped pair index, the bilinear form, the node weight) and the per-wave counting into the library's counter words.
// Host side, dimension-free: PtSet, a particle set in 2 or 3 axes (each file converts its jrx_particles2d / jrx_particles3d to it in one place, pt_geom / p3_geom);
// the checks of a set (pt_check_set); the overlap rules (pt_slots, pt_apart, pt_disjoint) on the primitives of op_args.hpp; the checks move_particles! and
// update_phase_ratios! make after the geometry (pt_move_checks, pt_ratio_checks); the counter read-back.  A file includes it inside no namespace of its own.
#ifndef JRX_PARTICLES_COMMON_HPP
#define JRX_PARTICLES_COMMON_HPP
#include <cfloat>
#include "op_args.hpp"

namespace {

__device__ __forceinline__ bool pt_finite(double v) { return fabs(v) <= DBL_MAX; }

// floor(s) as an index of the left node of an interpolation pair among m nodes: clamped on the double, so the pair exists and a point outside extrapolates
__device__ __forceinline__ int pt_pair(double s, int m)
{
    const double f = floor(s);
    return f >= 0.0 ? (f < (double)(m - 1) ? (int)f : m - 2) : 0;
}

// the bilinear form every interpolation here uses, in this order
__device__ __forceinline__ double pt_bilin(double tx, double ty, double v00, double v10, double v01, double v11)
{
    return (1.0 - ty) * ((1.0 - tx) * v00 + tx * v10) + ty * ((1.0 - tx) * v01 + tx * v11);
}

// the weight of a particle at coordinate x to a node at xn
__device__ __forceinline__ double pt_w(double x, double xn, double idx) { return 1.0 - fabs(x - xn) * idx; }

// sum of a per-thread count over the wave (blocks are 64 wide in x: a wave is one row of the tile); lane 0 holds it
__device__ __forceinline__ int pt_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ... added to *word by lane 0
__device__ __forceinline__ void pt_count(unsigned long long *word, int v)
{
    v = pt_wave_sum(v);
    if (threadIdx.x == 0 && v != 0) atomicAdd(word, (unsigned long long)v);
}

// ------------------------------------------------------------------------------------------------ host side
// a particle set as the checks see it: nd = 2 or 3 axes (0: the caller's struct was NULL); the device structs (PtGeom, P3Geom) are filled from the checked set
struct PtSet {
    int nd;
    const void *coord[3], *active;
    i64 n[3];
    int mx;                           // max_xcell
    double o[3], d[3], id[3];         // origin, spacing, inverse spacing
};

// the checks every entry point shares
jrx_status pt_check_set(jrx_handle *h, const char *fn, const char *what, const PtSet &S)
{
    static const char *const axis[3] = {"px", "py", "pz"};
    const int nd = S.nd;
    if (nd == 0) return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL", fn, what);
    for (int a = 0; a < nd; a++)
        if (!S.coord[a]) return jrx_fail(h, JRX_ERR_ARG, "%s: %s.%s is NULL", fn, what, axis[a]);
    if (!S.active) return jrx_fail(h, JRX_ERR_ARG, "%s: %s.active is NULL", fn, what);
    bool ok = true, fin = true, pos = true, inv = true;
    double slots = 1.0, nodes = 1.0;
    for (int a = 0; a < nd; a++) {
        ok = ok && S.n[a] >= 1;
        slots *= (double)S.n[a], nodes *= (double)(S.n[a] + 2);
        fin = fin && std::isfinite(S.o[a]);
        pos = pos && S.d[a] > 0.0 && std::isfinite(S.d[a]);
        inv = inv && S.id[a] == 1.0 / S.d[a];
    }
    if (!ok) return jrx_fail(h, JRX_ERR_ARG, "%s: %s has %s cells", fn, what, op_list(S.n, nd, " x ").s);
    if (S.mx < 1) return jrx_fail(h, JRX_ERR_ARG, "%s: %s.max_xcell = %d", fn, what, S.mx);
    // 32-bit offsets: into the particle arrays, and into the largest grid field (2D: a phase-ratio member, JRX_MAXPHASE values per node; 3D: a ghosted velocity)
    if (op_2g(slots * (double)S.mx) || op_2g(nd == 2 ? nodes * JRX_MAXPHASE : nodes))
        return jrx_fail(h, JRX_ERR_ARG, "%s: %s has 2^31 or more slots or nodes (32-bit offsets)", fn, what);
    // 3D launches put y and z on blockIdx.y and .z, two cells (or nodes) per block; the 2D launch grid is one-dimensional
    if (nd == 3 && (S.n[1] > 2 * 65535 - 2 || S.n[2] > 2 * 65535 - 2))
        return jrx_fail(h, JRX_ERR_ARG, "%s: %s has more than %d cells along y or z (the launch grid)", fn, what, 2 * 65535 - 2);
    if (!fin) return jrx_fail(h, JRX_ERR_ARG, "%s: %s has origin (%s) (must be finite)", fn, what, op_list(S.o, nd, ", ").s);
    if (!pos) return jrx_fail(h, JRX_ERR_ARG, "%s: %s has spacings (%s) (must be positive and finite: a uniform grid)", fn, what, op_list(S.d, nd, ", ").s);
    if (!inv)
        return jrx_fail(h, JRX_ERR_ARG, "%s: %s.%s = (%s) are not %s", fn, what, nd == 2 ? "_dx, ._dy" : "_dx, ._dy, ._dz", op_list(S.id, nd, ", ").s,
                        nd == 2 ? "1 / dx, 1 / dy" : "1 / dx, 1 / dy, 1 / dz");
    if (jrx_comm_active(h)) return jrx_fail(h, JRX_ERR_ARG, "%s: a handle with a communicator (particles are built for one block)", fn);
    return JRX_OK;
}

i64 pt_slots(const PtSet &S)
{
    i64 ns = S.mx;
    for (int a = 0; a < S.nd; a++) ns *= S.n[a];
    return ns;
}

// an array must not share memory with the coordinates or the mask of S
jrx_status pt_apart(jrx_handle *h, const char *fn, const OpArr &x, const PtSet &S)
{
    const i64 ns = pt_slots(S);
    bool hit = op_overlaps(x.p, x.bytes, S.active, 4 * ns);
    for (int a = 0; a < S.nd; a++) hit = hit || op_overlaps(x.p, x.bytes, S.coord[a], 8 * ns);
    if (hit) return jrx_fail(h, JRX_ERR_ARG, "%s: %s overlaps the particle coordinates or the mask", fn, x.name);
    return JRX_OK;
}

// every array present; no output shares memory with the particles' own arrays, an input or another output.  `two`: the sentence for two outputs that overlap,
// where the outputs do not carry names of their own
jrx_status pt_disjoint(jrx_handle *h, const char *fn, const OpArr *out, int nout, const OpArr *in, int nin, const PtSet &S, const char *two = nullptr)
{
    JRX_TRY(op_present(h, fn, out, nout));
    JRX_TRY(op_present(h, fn, in, nin));
    for (int m = 0; m < nout; m++) JRX_TRY(pt_apart(h, fn, out[m], S));
    const OpClash c = op_disjoint(out, nout, in, nin);
    if (!c) return JRX_OK;
    if (!c.two) return jrx_fail(h, JRX_ERR_ARG, "%s: %s overlaps %s", fn, out[c.a].name, in[c.b].name);
    return two ? jrx_fail(h, JRX_ERR_ARG, "%s: %s", fn, two) : jrx_fail(h, JRX_ERR_ARG, "%s: %s and %s overlap", fn, out[c.a].name, out[c.b].name);
}

// move_particles!, after the two geometries: the counters, the two sets alike, the particle fields, and nothing written -- the destination's arrays, its fields,
// the byte buffer `work` of the 3D move (NULL: none) -- sharing memory with anything read or with another output
jrx_status pt_move_checks(jrx_handle *h, const char *fn, const PtSet &S, const PtSet &D, const double *const *args_src, double *const *args_dst, int32_t nargs,
                          const void *work, const int64_t *counts)
{
    static const char *const source[JRX_MAXPHASE] = {"source particle field 1", "source particle field 2", "source particle field 3", "source particle field 4",
                                                     "source particle field 5", "source particle field 6", "source particle field 7", "source particle field 8"};
    if (!counts) return jrx_fail(h, JRX_ERR_ARG, "%s: counts is NULL", fn);
    bool alike = S.mx == D.mx;
    for (int a = 0; a < S.nd; a++) alike = alike && S.n[a] == D.n[a] && S.o[a] == D.o[a] && S.d[a] == D.d[a];
    if (!alike) return jrx_fail(h, JRX_ERR_ARG, "%s: source and destination differ in extents, max_xcell, origin or spacing", fn);
    if (nargs < 0 || nargs > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d particle fields (0 .. %d are built)", fn, (int)nargs, JRX_MAXPHASE);
    if (nargs > 0 && (!args_src || !args_dst)) return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL with %d particle fields", fn, !args_src ? "args_src" : "args_dst", (int)nargs);
    for (int k = 0; k < nargs; k++)
        if (!args_src[k] || !args_dst[k]) return jrx_fail(h, JRX_ERR_ARG, "%s: particle field %d (%s) is NULL", fn, k + 1, !args_src[k] ? "source" : "destination");
    const i64 ns = pt_slots(D);
    const char *dest = "an array of the destination";
    OpArr out[5 + JRX_MAXPHASE], in[JRX_MAXPHASE];
    int nout = 0;
    for (int a = 0; a < D.nd; a++) out[nout++] = OpArr{D.coord[a], 8 * ns, dest};
    out[nout++] = OpArr{D.active, 4 * ns, dest};
    for (int k = 0; k < nargs; k++) out[nout++] = OpArr{args_dst[k], 8 * ns, dest}, in[k] = OpArr{args_src[k], 8 * ns, source[k]};
    if (work) out[nout++] = OpArr{work, ns, "work"};
    return pt_disjoint(h, fn, out, nout, in, nargs, S, "two arrays of the destination overlap");
}

// update_phase_ratios!, after the geometry: member m, named names[m], holds nphase values on each node of the box of extents n + stag[m]
jrx_status pt_ratio_checks(jrx_handle *h, const char *fn, const PtSet &S, double *const *members, const char *const *names, const int (*stag)[3], int nm,
                           const double *pPhases, int32_t nphase, const int64_t *n_empty)
{
    if (!members) return jrx_fail(h, JRX_ERR_ARG, "%s: phase_ratios is NULL", fn);
    OpArr out[8];
    for (int m = 0; m < nm; m++) out[m] = OpArr{members[m], 0, names[m]};
    const OpArr in[1] = {{pPhases, 8 * pt_slots(S), "pPhases"}};
    JRX_TRY(op_present(h, fn, out, nm));
    JRX_TRY(op_present(h, fn, in, 1));
    if (!n_empty) return jrx_fail(h, JRX_ERR_ARG, "%s: n_empty is NULL", fn);
    if (nphase < 1 || nphase > JRX_MAXPHASE) return jrx_fail(h, JRX_ERR_ARG, "%s: %d phases (1 .. %d are built)", fn, (int)nphase, JRX_MAXPHASE);
    for (int m = 0; m < nm; m++) {
        out[m].bytes = 8 * (i64)nphase;
        for (int a = 0; a < S.nd; a++) out[m].bytes *= S.n[a] + stag[m][a];
    }
    return pt_disjoint(h, fn, out, nm, in, 1, S);
}

// the counter words: six 64-bit integers in the tail of the handle's reduction scratch (every entry point here is synchronous)
constexpr int kPtWord0 = 10;
unsigned long long *pt_words(jrx_handle *h) { return (unsigned long long *)(h->d_sums + kPtWord0); }

// words first .. first + n - 1 back to the host, after everything queued on the stream
jrx_status pt_read_words(jrx_handle *h, int first, int n, int64_t *out)
{
    JRX_HIP(h, hipMemcpyAsync(h->h_sums + kPtWord0 + first, h->d_sums + kPtWord0 + first, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(out, h->h_sums + kPtWord0 + first, sizeof(int64_t) * n);
    return JRX_OK;
}

}  // namespace
#endif
