// heat_plan.hpp -- the two decisions of the heat-diffusion drivers that need no device: which iterations of the PT loop somebody observes (heat_solve,
// thermal_common.hpp) and the tile of the 3D one-launch kernels (thermal3d.hip).  No HIP header: g++ alone compiles it (tests/host/heat_plan_harness.cpp).
#pragma once
#include <cstdint>
#include "pt_replay.hpp"

namespace heat_plan {

// Observed iterations (1-based): the multiples of nout (a residual check follows them) and the last one, iterMax.  Runs of unobserved iterations replay in
// whole graphs of kGraphIters (an even count: the ping-pong sets end where they began), the rest as single launches.
constexpr int kGraphIters = 32;
// the window itself is pt_replay's, with iterMax as the last iteration the loop can run
inline int64_t next_observed(int64_t iter, int64_t nout, int64_t iterMax) { return pt_replay::next_observed(iter, nout, iterMax); }
inline int64_t unobserved_run(int64_t iter, int64_t nout, int64_t iterMax) { return pt_replay::unobserved_run(iter, nout, iterMax); }
inline bool observes_next(int64_t iter, int64_t nout, int64_t iterMax) { return pt_replay::observes_next(iter, nout, iterMax); }

// Tile of k_thermal3d_fused: TX cells of R rows, KZ planes deep; ntx x nty x ntz tiles.  The tuning switch "thermal_cfg" = R*10000 + (TX/64)*100 + KZ overrides the default:
// TX by nx, one row, 4 planes, halved while the launch has fewer than 4096 waves -- a block marches its planes one after the other, and a small grid in 4-plane chunks leaves
// most of the chip idle (64^3: 1024 single-wave blocks): 16^3 74.7 k -> 175 k it/s, 32^3 72.4 k -> 159 k, 48^3 64.3 k -> 112 k, 64^3 52.5 k -> 101 k with one plane per block;
// from 96^3 on 4 planes are the better depth again (35.5 k against 33.2 k) (profiles/r03_small_grids_graphs.txt).  The shallower chunks are instantiated for the default XCD
// band width only: with the tuning switch "thermal_xg" != 8 the depth stays 4.
struct Tile3 { int TX, R, KZ, ntx, nty, ntz; };
inline Tile3 tile3d(int nx, int ny, int nz, int cfg, int xg)
{
    Tile3 t;
    t.TX = cfg ? ((cfg / 100) % 100) * 64 : (nx > 128 ? 256 : (nx > 64 ? 128 : 64));
    t.R = cfg ? cfg / 10000 : 1;
    t.KZ = cfg ? cfg % 100 : 4;
    if (!cfg && xg == 8)
        while (t.KZ > 1 && (int64_t)((nx + t.TX - 1) / t.TX) * (t.TX / 64) * ny * ((nz + t.KZ - 1) / t.KZ) < 4096) t.KZ /= 2;
    t.ntx = (nx + t.TX - 1) / t.TX; t.nty = (ny + t.R - 1) / t.R; t.ntz = (nz + t.KZ - 1) / t.KZ;
    return t;
}

// The instantiations the 3D dispatch builds, in the order it tries them: X(TX, KZ, R, XG) of k_thermal3d_fused<TX, KZ, XG, R>, and X(TX, KZ) of k_thermal3d_fused_ph<TX, KZ, 8, .>
// (the phase-ratio form fuses with the default plan only).  Measured at 256^3 (profiles/r01_thermal3d_fused_sweep.txt): one row per thread 2289 it/s, two rows 1526, four rows 1301.
#define HEAT3_FUSED_SHAPES(X)                                                                                                                     \
    X(256, 4, 1, 8) X(128, 4, 1, 8) X(64, 4, 1, 8) X(256, 8, 1, 8) X(256, 4, 2, 8)                                                                \
    X(256, 4, 1, 1) X(256, 4, 1, 2) X(256, 4, 1, 4) X(256, 2, 1, 1) X(256, 2, 1, 2) X(256, 8, 1, 1) X(128, 4, 1, 1) X(64, 4, 1, 1)                 \
    X(64, 2, 1, 8) X(64, 1, 1, 8) X(128, 2, 1, 8) X(128, 1, 1, 8) X(256, 2, 1, 8) X(256, 1, 1, 8)
#define HEAT3_FUSED_PH_SHAPES(X) X(256, 4) X(128, 4) X(64, 4) X(256, 2) X(128, 2) X(64, 2) X(256, 1) X(128, 1) X(64, 1)
inline bool fused_shape_built(const Tile3 &t, int xg)
{
#define X(TX_, KZ_, R_, XG_) if (t.TX == TX_ && t.KZ == KZ_ && t.R == R_ && xg == XG_) return true;
    HEAT3_FUSED_SHAPES(X)
#undef X
    return false;
}
inline bool fused_ph_shape_built(const Tile3 &t)
{
#define X(TX_, KZ_) if (t.TX == TX_ && t.KZ == KZ_ && t.R == 1) return true;
    HEAT3_FUSED_PH_SHAPES(X)
#undef X
    return false;
}

}   // namespace heat_plan
