// rotate_point.hpp -- the per-point 2D stress rotation shared by the grid form (stress_rotation.hip, k_rotate_stress2d) and the particle form (particles.hip,
// k_pt_rotate and k_pt_rotate_stress): one text, so both leave the same bits for the same operands.  include/jrx.h, "Rotation".
#pragma once
#include <hip/hip_runtime.h>

// METHOD 0: τ' = R (τ R') with R = [c -s; s c], θ = dt ω (stress_rotation_particles.jl:175-197); METHOD 1: τ + dt (W τ - τ W), the corrected Jaumann rate
template <int METHOD>
__device__ __forceinline__ void rs_rot2(double xx, double yy, double xy, double th, double &oxx, double &oyy, double &oxy)
{
    if (METHOD == 0) {
        double s, c;
        sincos(th, &s, &c);
        const double ms = -s;
        const double m11 = xx * c + xy * ms, m12 = xx * s + xy * c;          // τ R'
        const double m21 = xy * c + yy * ms, m22 = xy * s + yy * c;
        oxx = c * m11 + ms * m21;                                           // R (τ R')
        oxy = c * m12 + ms * m22;
        oyy = s * m12 + c * m22;
    } else {
        const double t2 = 2.0 * th;
        oxx = xx - t2 * xy;
        oyy = yy + t2 * xy;
        oxy = xy + th * (xx - yy);
    }
}
