// vep3_plan.hpp -- the launch plan of the 3D VEP driver (stokes3d_vep.hip): every size-dependent decision of its launches as plain functions of integers -- the form and
// tiling of the edge pass, the chunk depth of k_vep3_pre, the thread map of k_vep3_prec.  Host only and free of HIP (tests/host/vep3_plan_harness.cpp builds it with g++
// alone).  The launchers take a plan and pick the instantiation it names; a combination no kernel is built for is refused here, before anything is launched.
#pragma once
#include <cstdint>

// ---- edge pass (option "vep3_edges"): 0 one node per thread (k_vep3_edges; also the form more than 4 phases use), 1 the z-marching kernel with one family per block and
// the three blocks of a tile on one XCD, 2 the same kernel as one launch per family (A/B: the L2 sharing), 3 / 4 (default) the three family waves of a row as one workgroup
// sharing the centre / centre and shear operands through LDS, 6 the same with a fourth, publishing wave
struct Vep3EdgePlan {
    const char *refused;       // nullptr, or why no kernel is built for the combination (nothing may be launched)
    int form;                  // 0 = node kernel, else the z-marching form 1, 2, 3, 4, 6.  Softening laws run form 1 (k_vep3_edges_zf<16, NP, 2, true>) whatever z-marching form is asked for
    int kz, mb;                // planes per z chunk, min blocks per CU (form 1)
    bool peel;                 // the thin last lane segment goes to the node kernel in a launch of its own
    int rem;                   // node columns behind the last full segment (the peeled ones if peel)
    int nseg, ilim;            // lane segments of the z-marching launch and the node columns [0, ilim) they cover
    int nzc;                   // z chunks
    int ntxy, ntxy_l;          // tiles per z chunk: nseg * ceil((ny + 1) / 4) (four rows per block: forms 1, 2) and nseg * (ny + 1) (one row per workgroup: forms 3, 4, 6)
    int nt, nt_l;              // ... times nzc
    unsigned grid_f, grid_l;   // blocks of the one-dimensional launches, padded to whole rounds of the 8 XCDs: form 1 (three family blocks per tile) and forms 3, 4, 6
    unsigned peel_gx, peel_gy; // grid of the peel launch (64 x 4 threads: rem * (ny + 1) node columns by nz + 1 planes)
};

// loop: called by the solve loop -- the form of the edge pass then follows the grid size (the kernel-level entry points keep the form the switch names)
inline Vep3EdgePlan vep3_plan_edges(int nx, int ny, int nz, int nphase, bool soft, bool loop, int opt_edges, int opt_cfg, bool opt_peel)
{
    Vep3EdgePlan pl = {};
    if (opt_edges != 0 && opt_edges != 1 && opt_edges != 2 && opt_edges != 3 && opt_edges != 4 && opt_edges != 6) { pl.refused = "vep3_edges: no such form"; return pl; }
    // Small grids (the reference's own 3D tests run at 16^3 .. 32^3): the z-marching edge kernel has a few hundred blocks, each a chain of 16 dependent planes, and the
    // one-node-per-thread kernel is the faster form -- 16^3 14.1 k -> 19.4 k it/s, 32^3 13.0 k -> 18.1 k, 48^3 10.5 k -> 12.4 k; equal at 56^3, z-marching from there on
    // (scripts/bench_vep3d_sizes.py, profiles/r03_vep3d_small_grids.txt)
    const int edges = (loop && opt_edges == 4 && (double)(nx + 1) * (ny + 1) * (nz + 1) <= 125000.0) ? 0 : opt_edges;
    if (edges == 0 || nphase > 4) return pl;       // form 0
    pl.form = soft ? 1 : edges;
    const int cfg = opt_cfg ? opt_cfg : 162;           // option "vep3_cfg" = KZ * 10 + min blocks per CU (tuning); 0: KZ by the grid size (below)
    int kz = cfg / 10;
    pl.mb = soft ? 2 : cfg % 10;
    // lane segments of 62 node columns; a last segment that would be less than 40 % full (256^3: 257 = 4 x 62 + 9) is not launched -- its node columns
    // go to the one-node-per-thread kernel in a thin launch of their own (the two launches write disjoint nodes and read old values only)
    const int nfull = (nx + 1) / 62, rem = (nx + 1) - 62 * nfull;
    // (a thin last segment is only worth a launch of its own behind at least two full ones: 72^3 6.9 k -> 7.3 k, 80^3 5.5 k -> 6.4 k it/s without it, 128^3 2.03 k with against 1.98 k without)
    // The peeled columns are independent of the main launch, but running the thin, load-instruction-bound node kernel (0.14 ms for 3.5 % of the nodes at 256^3) on a second stream
    // beside the main kernel measured 266.1 / 267.6 it/s against 269.2 / 269.8 in order (256^3, same box, alternating): it follows on the same stream
    pl.rem = rem; pl.peel = nfull >= 2 && rem > 0 && rem <= 24 && opt_peel;
    pl.nseg = pl.peel ? nfull : (nx + 1 + 61) / 62; pl.ilim = pl.peel ? 62 * nfull : nx + 1;
    // chunk depth of the LDS-sharing form: 16 planes where that gives the chip enough blocks, halved (down to 4) while the launch has fewer than 3000 -- 56^3 12.6 k -> 15.6 k it/s,
    // 64^3 9.6 k -> 10.7 k, 96^3 4.12 k -> 4.33 k, 128^3 +1.4 %; from 160^3 on 16 planes are the best (profiles/r03_vep3d_small_grids.txt)
    if (!opt_cfg && edges == 4 && !soft)
        while (kz > 4 && (int64_t)pl.nseg * (ny + 1) * ((nz + kz) / kz) < 3000) kz /= 2;
    pl.kz = kz;
    // the instantiations that are built
    const bool built = pl.form == 1 ? (soft ? kz == 16 : ((kz == 16 && (pl.mb == 2 || pl.mb == 3)) || (kz == 8 && pl.mb == 2)))
                     : pl.form == 4 ? (kz == 16 || kz == 8 || kz == 4)
                                    : kz == 16;
    if (!built) { pl.refused = "vep3_cfg: no such configuration"; return pl; }
    pl.nzc = (nz + 1 + kz - 1) / kz;
    pl.ntxy = pl.nseg * ((ny + 1 + 3) / 4); pl.ntxy_l = pl.nseg * (ny + 1);
    pl.nt = pl.ntxy * pl.nzc; pl.nt_l = pl.ntxy_l * pl.nzc;
    pl.grid_f = (unsigned)(((pl.nt + 7) / 8) * 8 * 3); pl.grid_l = (unsigned)(((pl.nt_l + 7) / 8) * 8);
    if (pl.peel) { pl.peel_gx = (unsigned)(((int64_t)pl.rem * (ny + 1) + 63) / 64); pl.peel_gy = (unsigned)((nz + 1 + 3) / 4); }
    return pl;
}

// ---- planes per thread of k_vep3_pre and k_vep3_prec (option "vep3_prekz"; 0: by the grid): 8 where that gives the chip enough blocks, halved while the launch has fewer than
// 2048 (16^3: 19.3 k -> 26.0 k it/s with one plane per thread, 32^3 18.1 k -> 23.3 k, 64^3 8.2 k -> 9.0 k, 128^3 +1 % with four; 256^3: eight planes stay the best, 318 against
// 304 it/s with one; profiles/r03_vep3d_small_grids.txt)
inline int vep3_plan_prekz(int nx, int ny, int nz, int opt_prekz)
{
    if (opt_prekz != 0) return opt_prekz;
    const int64_t gx = ((int64_t)(nx + 1) * (ny + 1) + 255) / 256;
    int prekz = 8;
    while (prekz > 1 && gx * ((nz + prekz) / prekz) < 2048) prekz /= 2;
    return prekz;
}
// k_vep3_pre takes the depth as a template argument: 1, 2, 4, 8, 16, 32 are built, any other value runs 8
inline int vep3_pre_depth(int prekz) { return (prekz == 1 || prekz == 2 || prekz == 4 || prekz == 16 || prekz == 32) ? prekz : 8; }

// ---- thread map of the fused kernel k_vep3_prec: 64 x 4 tiles of node columns where a plane has enough of them ("vep3_prec_tile" = 2, default: from 16,384 node columns per plane),
// else 256 consecutive nodes of the flattened plane.  With tiles the rows of a velocity / η window that a block's rows share are requested by waves of one block: 35.4 -> 30.1 fetched
// passes, 256^3 350 -> 365 it/s (128^3 +3 %, 160^3 +4 %, 224^3 +5 %, 320^3 +2 %); on small planes the partly filled tiles cost more: 96^3 -7 %, 64^3 -8 %, 32^3 -6 % (profiles/r04_vep3d_fused_pre_centre.txt, section 7)
struct Vep3PrecPlan {
    int kz;             // planes per thread
    int tntx;           // tiles per row of node columns, 0 = the flattened map
    unsigned gx, gy;    // grid
};
inline Vep3PrecPlan vep3_plan_prec(int nx, int ny, int nz, int kz, int opt_tile)
{
    Vep3PrecPlan pl;
    pl.kz = kz;
    const bool tiled = opt_tile == 1 || (opt_tile == 2 && (int64_t)(nx + 1) * (ny + 1) >= 16384);
    pl.tntx = tiled ? (nx + 1 + 63) / 64 : 0;
    pl.gx = tiled ? (unsigned)(pl.tntx * ((ny + 1 + 3) / 4)) : (unsigned)(((int64_t)(nx + 1) * (ny + 1) + 255) / 256);
    pl.gy = (unsigned)((nz + 1 + kz - 1) / kz);
    return pl;
}
