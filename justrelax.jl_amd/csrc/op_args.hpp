// op_args.hpp -- the host checks the synchronous operator entry points share (the grid operators advection, phase_ratios, stress_rotation, topography,
// principal, stepops, gridops .hip and, through particles_common.hpp, the particles): arrays named for the messages, "every array present", "no output
// shares memory with an input or another output", extents, the 2^31 bound of the 32-bit offsets, finiteness, the "5 x 4 x 3" spellings, and the end of a
// call (launch check, synchronise).  The primitives find; the caller words the refusal, since the sentences differ from operator to operator.
// An entry point checks in this order: NULL arguments, enumerations, extents, 2^31, finiteness, overlap, and last jrx_check_device -- so a call with bad
// arguments is refused without touching the HIP runtime.  A file includes this inside no namespace of its own.
#ifndef JRX_OP_ARGS_HPP
#define JRX_OP_ARGS_HPP
#include <initializer_list>
#include "jrx_internal.hpp"

namespace {

// the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte
bool op_overlaps(const void *a, i64 abytes, const void *b, i64 bbytes)
{
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

// an array as the checks see it; name: what a message calls it
struct OpArr {
    const void *p;
    i64 bytes;
    const char *name;
};

jrx_status op_present(jrx_handle *h, const char *fn, const OpArr *x, int n)
{
    for (int m = 0; m < n; m++)
        if (!x[m].p) return jrx_fail(h, JRX_ERR_ARG, "%s: %s is NULL", fn, x[m].name);
    return JRX_OK;
}

// the first pair that shares memory: out[a] with in[b], or (two) with out[b]; a < 0: none
struct OpClash {
    int a, b;
    bool two;
    explicit operator bool() const { return a >= 0; }
};

// The search order, the same for every caller: for each output in list order, the inputs in list order, then the later outputs.  Inputs may share memory
// among themselves (they are only read).
OpClash op_disjoint(const OpArr *out, int nout, const OpArr *in, int nin)
{
    for (int m = 0; m < nout; m++) {
        for (int k = 0; k < nin; k++)
            if (op_overlaps(out[m].p, out[m].bytes, in[k].p, in[k].bytes)) return {m, k, false};
        for (int q = m + 1; q < nout; q++)
            if (op_overlaps(out[m].p, out[m].bytes, out[q].p, out[q].bytes)) return {m, q, true};
    }
    return {-1, -1, false};
}

// every one of the nd extents >= 1
bool op_extents_ok(const int64_t *n, int nd)
{
    bool ok = true;
    for (int d = 0; d < nd; d++) ok = ok && n[d] >= 1;
    return ok;
}

// the entries of the n .+ pad box as a double: exact far beyond 2^31, never overflows
double op_count(const int64_t *n, int nd, int pad)
{
    double c = 1.0;
    for (int d = 0; d < nd; d++) c *= (double)n[d] + (double)pad;
    return c;
}

// an array of so many entries is beyond the 32-bit element offsets of the kernels
bool op_2g(double entries) { return entries >= 2147483648.0; }

// the bytes of an array of doubles with n[d] + pad[d] entries along axis d (checked extents: the product fits)
i64 op_bytes(const int64_t *n, int nd, int p0, int p1, int p2 = 0)
{
    const int pad[3] = {p0, p1, p2};
    i64 b = 8;
    for (int d = 0; d < nd; d++) b *= n[d] + pad[d];
    return b;
}

// ... of component c of a staggered velocity with its ghost layers: n + 1 entries along c, n + 2 along the other axes
i64 op_vel_bytes(const int64_t *n, int nd, int c) { return op_bytes(n, nd, c == 0 ? 1 : 2, c == 1 ? 1 : 2, c == 2 ? 1 : 2); }

bool op_pos_finite(double x) { return x > 0.0 && x <= 1.79769313486231570e308; }

bool op_finite(std::initializer_list<double> v)
{
    bool ok = true;
    for (double x : v) ok = ok && std::isfinite(x);
    return ok;
}

// the first nd entries of v as text: "7 x 5" or "0.25, -0.5"
struct OpText {
    char s[112];
};
template <typename T>
OpText op_list(const T *v, int nd, const char *sep)
{
    OpText t = {};
    for (int a = 0, at = 0; a < nd; a++)
        at += std::is_integral<T>::value ? snprintf(t.s + at, sizeof t.s - at, "%s%lld", a ? sep : "", (long long)v[a])
                                         : snprintf(t.s + at, sizeof t.s - at, "%s%g", a ? sep : "", (double)v[a]);
    return t;
}

// the end of a synchronous entry point: what was launched is checked and waited for
jrx_status op_finish(jrx_handle *h)
{
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

}  // namespace
#endif
