// edge_stencils3d.hpp -- the clamped gather tables of update_stresses_center_vertex_ps! 3D (src/stokes/StressKernels.jl:604-668), shared by the 3D
// visco-elasto-plastic kernels (stokes3d_vep.hip) and the 3D DYREL stress kernel (dyrel3d.hip).
#pragma once

namespace {

// Stencil tables of StressKernels.jl:604-668 for the edge families T = 0 (yz), 1 (xz), 2 (xy): entries pick the
// clamped index {0: n-1, 1: n, 2: n+1} per direction, in the reference's order of summation.  constexpr functions so that the
// unrolled loops fold every table entry into the address arithmetic.
// cen3(T, q, d): cell q of the four centres around an edge of family T (av_clamped_yz / _xz / _xy, harm_clamped_*)
__host__ __device__ constexpr int cen3(int t, int q, int d)
{
    constexpr int T[3][4][3] = {
        {{1, 0, 0}, {1, 1, 0}, {1, 0, 1}, {1, 1, 1}},
        {{0, 1, 0}, {1, 1, 0}, {0, 1, 1}, {1, 1, 1}},
        {{0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}}};
    return T[t][q][d];
}
// oth3(T, s, q, d): node q of the four edges of family s around an edge of family T (av_clamped_yz_y / _z, ... _xy_x / _y)
__host__ __device__ constexpr int oth3(int t, int s, int q, int d)
{
    constexpr int T[3][3][4][3] = {
        {{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, {{1, 0, 1}, {2, 0, 1}, {1, 1, 1}, {2, 1, 1}}, {{1, 1, 0}, {2, 1, 0}, {1, 1, 1}, {2, 1, 1}}},
        {{{0, 1, 1}, {1, 1, 1}, {1, 2, 1}, {0, 2, 1}}, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, {{1, 1, 0}, {1, 2, 0}, {1, 1, 1}, {1, 2, 1}}},
        {{{0, 1, 1}, {1, 1, 1}, {0, 1, 2}, {1, 1, 2}}, {{1, 0, 1}, {1, 1, 1}, {1, 0, 2}, {1, 1, 2}}, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}}};
    return T[t][s][q][d];
}

}   // namespace
