// particles_common.hpp -- what the 2D (particles.hip) and the 3D (particles3d.hip) particle kernels share: the per-axis pieces of every definition of
// include/jrx.h (the finite test, the clamped pair index, the bilinear form, the node weight), the per-wave counting into the library's counter words, and the
// host-side overlap test and counter read-back.  Everything here is dimension-free; a file includes it inside no namespace of its own.
#ifndef JRX_PARTICLES_COMMON_HPP
#define JRX_PARTICLES_COMMON_HPP
#include <cfloat>
#include "jrx_internal.hpp"

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

bool pt_overlaps(const void *a, i64 abytes, const void *b, i64 bbytes)
{
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

struct PtArr {
    const void *p;
    i64 bytes;
    const char *name;
};

// the counter words: six 64-bit integers in the tail of the handle's reduction scratch (every entry point here is synchronous)
unsigned long long *pt_words(jrx_handle *h) { return (unsigned long long *)(h->d_sums + 10); }

jrx_status pt_read_words(jrx_handle *h, int n, int64_t *out)
{
    JRX_HIP(h, hipMemcpyAsync(h->h_sums + 10, h->d_sums + 10, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    memcpy(out, h->h_sums + 10, sizeof(int64_t) * n);
    return JRX_OK;
}

jrx_status pt_finish(jrx_handle *h)
{
    JRX_LAUNCH_CHECK(h);
    JRX_HIP(h, hipStreamSynchronize(h->stream));
    return JRX_OK;
}

}  // namespace
#endif
