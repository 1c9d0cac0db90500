// op_refusals_harness.cpp -- the refusals of the 31 grid-operator entry points (advection, phase_ratios, stress_rotation, topography, principal, stepops,
// gridops .hip), pinned on the host: for every entry point one valid call, one call per refusal site with exactly one fault, and the edge cases of the shared
// check layer (csrc/op_args.hpp); then a few 2D and 3D particle calls, whose checks stand on the same layer.  Prints one line per scenario: entry point | scenario | status | text; tests/test_host_op_refusals.py compares the output with
// tests/host/op_refusals_expected.txt.
//
// No HIP runtime call is made: jrx_check_device is a stub that always fails with a sentinel text, so a call whose arguments pass every check ends there, and the
// arrays are addresses that nothing dereferences.  The program behaves the same with or without a GPU.
#include <cstdint>
#include <cstdio>
#include "jrx_internal.hpp"

char g_jrx_create_err[512];
static bool g_comm = false;        // a scenario sets it to reach the refusals that ask for a communicator
bool jrx_comm_active(const jrx_handle *) { return g_comm; }
bool jrx_comm_has_neighbor(const jrx_handle *, int, int) { return g_comm; }
jrx_status jrx_check_device(jrx_handle *h) { return jrx_fail(h, JRX_ERR_HIP, "reached the device check"); }

namespace {

jrx_handle H;
const char *g_entry = "";
int g_lines = 0;

void rep(const char *scenario, jrx_status st)
{
    printf("%s | %s | %d | %s\n", g_entry, scenario, (int)st, H.err);
    H.err[0] = 0;
    g_lines++;
}

// array k: an address nothing dereferences, 2^45 bytes from its neighbours (the largest array here, 3 x (2^39 - 1) doubles, is below that); off in bytes
double *A(int k, int64_t off = 0) { return (double *)(uintptr_t)((1ull << 52) + ((uint64_t)k << 45) + (uint64_t)off); }

constexpr int64_t NX = 5, NY = 4, NZ = 3;
constexpr int64_t k2G = 2147483648ll;       // 2^31
const double kNaN = std::nan(""), kInf = INFINITY;

#define CASE(name, ...)         \
    {                           \
        auto a = good;          \
        __VA_ARGS__;            \
        rep(name, call(a));     \
    }

// ------------------------------------------------------------------------------------------------ topography.hip
void topography()
{
    {
        g_entry = "jrx_compute_rock_fraction2d";
        struct { double *c, *v, *vx, *vy; const double *h; int64_t nx, ny; double y0, idy; } good = {A(0), A(1), A(2), A(3), A(4), NX, NY, -1.0, 4.0};
        auto call = [](auto &a) { return jrx_compute_rock_fraction2d(&H, a.c, a.v, a.vx, a.vy, a.h, a.nx, a.ny, a.y0, a.idy); };
        const int64_t nc = 8 * NX * NY, nv = 8 * (NX + 1) * (NY + 1), nh = 8 * (NX + 1);
        CASE("valid", )
        CASE("center NULL", a.c = nullptr)
        CASE("Vy NULL", a.vy = nullptr)
        CASE("topo.h NULL", a.h = nullptr)
        CASE("nx = 0", a.nx = 0)
        CASE("box at 2^31", a.nx = 65534; a.ny = 32766)
        CASE("y0 NaN", a.y0 = kNaN)
        CASE("_dy Inf", a.idy = kInf)
        CASE("vertex overlaps topo.h", a.v = A(4))
        CASE("center and Vy overlap", a.vy = A(0))
        CASE("edge: vertex right behind center", a.v = A(0, nc))
        CASE("edge: center right behind vertex", a.c = A(1, nv))
        CASE("edge: vertex starts on the last entry of center", a.v = A(0, nc - 8))
        CASE("edge: vertex ends on the first entry of center", a.v = A(0, -(nv - 8)))
        CASE("edge: topo.h right behind Vy", a.h = A(3, 8 * NX * (NY + 1)))
        CASE("edge: topo.h ends on the first entry of center", a.h = A(0, -(nh - 8)))
    }
    {
        g_entry = "jrx_advect_topography2d";
        struct { double *h, *ho; const double *vx, *vy; int64_t nx, ny; double y0, idx, idy, dt; } good = {A(0), A(1), A(2), A(3), NX, NY, -1.0, 5.0, 4.0, 0.1};
        auto call = [](auto &a) { return jrx_advect_topography2d(&H, a.h, a.ho, a.vx, a.vy, a.nx, a.ny, a.y0, a.idx, a.idy, a.dt); };
        CASE("valid", )
        CASE("topo.h NULL", a.h = nullptr)
        CASE("topo.h_old NULL", a.ho = nullptr)
        CASE("V.Vx NULL", a.vx = nullptr)
        CASE("V.Vy NULL", a.vy = nullptr)
        CASE("ny = -1", a.ny = -1)
        CASE("box at 2^31", a.nx = 65534; a.ny = 32766)
        CASE("dt NaN", a.dt = kNaN)
        CASE("topo.h overlaps topo.h_old", a.ho = A(0))
        CASE("topo.h overlaps V.Vy", a.h = A(3, 8))
        CASE("topo.h_old overlaps V.Vx", a.ho = A(2, 16))
        CASE("valid: V.Vx and V.Vy the same array", a.vy = A(2))
    }
    {
        g_entry = "jrx_update_phases_topography2d";
        double *ph[3] = {A(0), A(1), A(2)};
        struct { double *const *ph; int32_t np; const double *h; int64_t nx, ny; double y0, idy; int32_t air; } good = {ph, 3, A(4), NX, NY, -1.0, 4.0, 3};
        auto call = [](auto &a) { return jrx_update_phases_topography2d(&H, a.ph, a.np, a.h, a.nx, a.ny, a.y0, a.idy, a.air); };
        double *null2[3] = {A(0), nullptr, A(2)}, *same[3] = {A(0), A(1), A(0, 8)}, *onh[3] = {A(0), A(4), A(2)};
        CASE("valid", )
        CASE("phases NULL", a.ph = nullptr)
        CASE("nphase = 0", a.np = 0)
        CASE("nphase = 9", a.np = 9)
        CASE("air_phase = 4 of 3", a.air = 4)
        CASE("phase field 2 NULL", a.ph = null2)
        CASE("topo.h NULL", a.h = nullptr)
        CASE("nx = 0", a.nx = 0)
        CASE("box at 2^31", a.nx = 65534; a.ny = 32766)
        CASE("y0 Inf", a.y0 = kInf)
        CASE("phase field 2 overlaps topo.h", a.ph = onh)
        CASE("phase fields 1 and 3 overlap", a.ph = same)
    }
    {
        g_entry = "jrx_compute_rock_fraction3d";
        struct { double *o[8]; const double *h; int64_t nx, ny, nz; double z0, idz; } good = {{A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7)}, A(8), NX, NY, NZ, -1.0, 4.0};
        auto call = [](auto &a) {
            return jrx_compute_rock_fraction3d(&H, a.o[0], a.o[1], a.o[2], a.o[3], a.o[4], a.o[5], a.o[6], a.o[7], a.h, a.nx, a.ny, a.nz, a.z0, a.idz);
        };
        const int64_t nc = 8 * NX * NY * NZ, nxy = 8 * (NX + 1) * (NY + 1) * NZ, nh = 8 * (NX + 1) * (NY + 1);
        CASE("valid", )
        CASE("center NULL", a.o[0] = nullptr)
        CASE("xy NULL", a.o[7] = nullptr)
        CASE("topo.h NULL", a.h = nullptr)
        CASE("nz = 0", a.nz = 0)
        CASE("box at 2^31", a.nx = 2046; a.ny = 1022; a.nz = 1022)
        CASE("z0 NaN", a.z0 = kNaN)
        CASE("xz overlaps topo.h", a.o[6] = A(8))
        CASE("Vx and xy overlap", a.o[7] = A(2, 8))
        CASE("edge: xy right behind center", a.o[7] = A(0, nc))
        CASE("edge: center right behind xy", a.o[0] = A(7, nxy))
        CASE("edge: xy starts on the last entry of center", a.o[7] = A(0, nc - 8))
        CASE("edge: xy ends on the first entry of center", a.o[7] = A(0, -(nxy - 8)))
        CASE("edge: topo.h right behind center", a.h = A(0, nc))
        CASE("edge: topo.h ends on the first entry of center", a.h = A(0, -(nh - 8)))
    }
    {
        g_entry = "jrx_advect_topography3d";
        struct { double *h, *ho; const double *vx, *vy, *vz; int64_t nx, ny, nz; double z0, idx, idy, idz, dt; } good = {A(0), A(1), A(2), A(3), A(4), NX, NY, NZ,
                                                                                                                         -1.0, 5.0, 4.0, 3.0, 0.1};
        auto call = [](auto &a) { return jrx_advect_topography3d(&H, a.h, a.ho, a.vx, a.vy, a.vz, a.nx, a.ny, a.nz, a.z0, a.idx, a.idy, a.idz, a.dt); };
        CASE("valid", )
        CASE("topo.h NULL", a.h = nullptr)
        CASE("topo.h_old NULL", a.ho = nullptr)
        CASE("V.Vx NULL", a.vx = nullptr)
        CASE("V.Vy NULL", a.vy = nullptr)
        CASE("V.Vz NULL", a.vz = nullptr)
        CASE("ny = 0", a.ny = 0)
        CASE("box at 2^31", a.nx = 2046; a.ny = 1022; a.nz = 1022)
        CASE("_dz Inf", a.idz = kInf)
        CASE("topo.h overlaps V.Vz", a.h = A(4, 8))
        CASE("topo.h_old overlaps V.Vy", a.ho = A(3, 8))
    }
    {
        g_entry = "jrx_update_phases_topography3d";
        double *ph[2] = {A(0), A(1)};
        struct { double *const *ph; int32_t np; const double *h; int64_t nx, ny, nz; double z0, idz; int32_t air; } good = {ph, 2, A(4), NX, NY, NZ, -1.0, 4.0, 1};
        auto call = [](auto &a) { return jrx_update_phases_topography3d(&H, a.ph, a.np, a.h, a.nx, a.ny, a.nz, a.z0, a.idz, a.air); };
        double *null1[2] = {nullptr, A(1)}, *same[2] = {A(0), A(0, 8 * (NX * NY * NZ - 1))}, *onh[2] = {A(4, 8), A(1)};
        CASE("valid", )
        CASE("phases NULL", a.ph = nullptr)
        CASE("nphase = 0", a.np = 0)
        CASE("air_phase = 0", a.air = 0)
        CASE("phase field 1 NULL", a.ph = null1)
        CASE("topo.h NULL", a.h = nullptr)
        CASE("nz = 0", a.nz = 0)
        CASE("box at 2^31", a.nx = 2046; a.ny = 1022; a.nz = 1022)
        CASE("_dz NaN", a.idz = kNaN)
        CASE("phase field 1 overlaps topo.h", a.ph = onh)
        CASE("phase fields 1 and 2 overlap", a.ph = same)
    }
}

// ------------------------------------------------------------------------------------------------ advection.hip
void advection()
{
    static const int64_t u2[2] = {NX, NY}, vx2[2] = {NX, NY + 1}, w2[2] = {NX + 1, NY}, zero2[2] = {NX, 0}, small2[2] = {NX, NY - 1};
    static const int64_t below2[2] = {k2G - 1, 1}, at2[2] = {k2G, 1};
    {
        g_entry = "jrx_weno5_advection2d";
        H.weno_fused = true;
        struct { double *u; const int64_t *ud; const double *vx; const int64_t *vxd; const double *vy; const int64_t *vyd; double *ut, *f[4]; const int64_t *wd;
                 double dx, dy, dt; int32_t method; } good = {A(0), u2, A(1), vx2, A(2), u2, A(3), {A(4), A(5), A(6), A(7)}, w2, 0.2, 0.25, 0.01, 2};
        auto call = [](auto &a) {
            return jrx_weno5_advection2d(&H, a.u, a.ud, a.vx, a.vxd, a.vy, a.vyd, a.ut, a.f[0], a.f[1], a.f[2], a.f[3], a.wd, a.dx, a.dy, a.dt, a.method);
        };
        CASE("valid", )
        CASE("u NULL", a.u = nullptr)
        CASE("fT NULL", a.f[3] = nullptr)
        CASE("wdim NULL", a.wd = nullptr)
        CASE("method = 3", a.method = 3)
        CASE("size(u) has a zero", a.ud = zero2; a.vxd = zero2; a.vyd = zero2; a.wd = zero2)
        CASE("vy smaller than u along 2", a.vyd = small2)
        CASE("weno arrays smaller than u along 2", a.wd = small2)
        CASE("edge: every array one below 2^31 entries", a.ud = below2; a.vxd = below2; a.vyd = below2; a.wd = below2)
        CASE("edge: vx at 2^31 entries", a.ud = below2; a.vxd = at2; a.vyd = below2; a.wd = below2)
        CASE("edge: the weno arrays at 2^31 entries", a.ud = below2; a.vxd = below2; a.vyd = below2; a.wd = at2)
        CASE("u and fB overlap", a.f[2] = A(0, 8))
        CASE("vx and ut overlap", a.ut = A(1, 8))
        CASE("fL and fR overlap", a.f[1] = A(4))
        CASE("valid: vx and vy the same array", a.vy = A(1))
        CASE("edge: ut right behind u", a.ut = A(0, 8 * NX * NY))
        CASE("edge: ut ends on the first entry of u", a.ut = A(0, -8 * ((NX + 1) * NY - 1)))
    }
    static const int64_t u3[3] = {NX, NY, NZ}, v3[3] = {NX + 1, NY, NZ}, w3[3] = {NX, NY + 1, NZ}, zero3[3] = {NX, NY, 0}, small3[3] = {NX, NY, NZ - 1};
    static const int64_t below3[3] = {k2G - 1, 1, 1}, at3[3] = {k2G, 1, 1};
    {
        g_entry = "jrx_weno5_advection3d";
        struct { double *u; const int64_t *ud; const double *vx; const int64_t *vxd; const double *vy; const int64_t *vyd; const double *vz; const int64_t *vzd;
                 double *ut, *f[6]; const int64_t *wd; double dx, dy, dz, dt; int32_t method; } good = {A(0), u3, A(1), v3, A(2), u3, A(3), u3, A(4),
                                                                                                       {A(5), A(6), A(7), A(8), A(9), A(10)}, w3, 0.2, 0.25, 0.3, 0.01, 1};
        auto call = [](auto &a) {
            return jrx_weno5_advection3d(&H, a.u, a.ud, a.vx, a.vxd, a.vy, a.vyd, a.vz, a.vzd, a.ut, a.f[0], a.f[1], a.f[2], a.f[3], a.f[4], a.f[5], a.wd, a.dx, a.dy,
                                         a.dz, a.dt, a.method);
        };
        CASE("valid", )
        CASE("vz NULL", a.vz = nullptr)
        CASE("fL NULL", a.f[0] = nullptr)
        CASE("vzdim NULL", a.vzd = nullptr)
        CASE("valid: fused form without fR .. fU", for (int q = 1; q < 6; q++) a.f[q] = nullptr)
        CASE("valid: fused form without fD", a.f[4] = nullptr)
        H.weno_fused = false;
        CASE("valid: per-kernel form", )
        CASE("per-kernel form without fD", a.f[4] = nullptr)
        H.weno_fused = true;
        CASE("method = 0", a.method = 0)
        CASE("size(u) has a zero", a.ud = zero3; a.vxd = zero3; a.vyd = zero3; a.vzd = zero3; a.wd = zero3)
        CASE("vz smaller than u along 3", a.vzd = small3)
        CASE("edge: every array one below 2^31 entries", a.ud = below3; a.vxd = below3; a.vyd = below3; a.vzd = below3; a.wd = below3)
        CASE("edge: vz at 2^31 entries", a.ud = below3; a.vxd = below3; a.vyd = below3; a.vzd = at3; a.wd = below3)
        CASE("edge: the weno arrays at 2^31 entries, fU absent", a.ud = below3; a.vxd = below3; a.vyd = below3; a.vzd = below3; a.wd = at3; a.f[5] = nullptr)
        CASE("u and fU overlap", a.f[5] = A(0, 8))
        CASE("vz and fL overlap", a.f[0] = A(3, 8))
        CASE("valid: vx, vy and vz the same array", a.vy = A(1); a.vz = A(1); a.vyd = v3; a.vzd = v3)
        CASE("edge: fL right behind ut", a.f[0] = A(4, 8 * NX * (NY + 1) * NZ))
        CASE("edge: fL starts on the last entry of ut", a.f[0] = A(4, 8 * (NX * (NY + 1) * NZ - 1)))
    }
}

// ------------------------------------------------------------------------------------------------ principal.hip
void principal()
{
    {
        g_entry = "jrx_principal_stresses2d";
        struct { double *s1, *s2; const double *xx, *yy, *xy; int64_t nx, ny; } good = {A(0), A(1), A(2), A(3), A(4), NX, NY};
        auto call = [](auto &a) { return jrx_principal_stresses2d(&H, a.s1, a.s2, a.xx, a.yy, a.xy, a.nx, a.ny); };
        CASE("valid", )
        CASE("σ2 NULL", a.s2 = nullptr)
        CASE("xy_c NULL", a.xy = nullptr)
        CASE("ny = 0", a.ny = 0)
        CASE("edge: one below 2^39 cells", a.nx = (1ll << 39) - 1; a.ny = 1)
        CASE("edge: 2^39 cells", a.nx = 1ll << 20; a.ny = 1ll << 19)
        CASE("σ1 and σ2 overlap", a.s2 = A(0, 8 * (2 * NX * NY - 1)))
        CASE("edge: σ2 right behind σ1", a.s2 = A(0, 8 * 2 * NX * NY))
        CASE("σ2 overlaps yy", a.yy = A(1, 8))
        CASE("edge: xx right behind σ1", a.xx = A(0, 8 * 2 * NX * NY))
        CASE("edge: xx ends on the first entry of σ1", a.xx = A(0, -8 * (NX * NY - 1)))
    }
    {
        g_entry = "jrx_principal_stresses3d";
        struct { double *s[3]; const double *t[6]; int64_t nx, ny, nz; } good = {{A(0), A(1), A(2)}, {A(3), A(4), A(5), A(6), A(7), A(8)}, NX, NY, NZ};
        auto call = [](auto &a) { return jrx_principal_stresses3d(&H, a.s[0], a.s[1], a.s[2], a.t[0], a.t[1], a.t[2], a.t[3], a.t[4], a.t[5], a.nx, a.ny, a.nz); };
        CASE("valid", )
        CASE("σ3 NULL", a.s[2] = nullptr)
        CASE("xz_c NULL", a.t[4] = nullptr)
        CASE("nz = 0", a.nz = 0)
        CASE("edge: one below 2^39 cells", a.nx = (1ll << 39) - 1; a.ny = 1; a.nz = 1)
        CASE("edge: 2^39 cells", a.nx = 1ll << 13; a.ny = 1ll << 13; a.nz = 1ll << 13)
        CASE("σ2 and σ3 overlap", a.s[2] = A(1, 8))
        CASE("σ3 overlaps xy_c", a.t[5] = A(2, 8 * (3 * NX * NY * NZ - 1)))
        CASE("edge: xy_c right behind σ3", a.t[5] = A(2, 8 * 3 * NX * NY * NZ))
    }
}

// ------------------------------------------------------------------------------------------------ stepops.hip
void stepops()
{
    jrx_rheology rh = {};
    rh.nphase = 2, rh.G[0] = 1.0, rh.G[1] = 2.0;
    jrx_rheology rh0 = rh, rh9 = rh;
    rh0.nphase = 0, rh9.nphase = 9;
    {
        g_entry = "jrx_pureshear_bc2d";
        struct { double *vx, *vy; const double *xv, *yv; double e; int64_t nx, ny; } good = {A(0), A(1), A(2), A(3), 1.0, NX, NY};
        auto call = [](auto &a) { return jrx_pureshear_bc2d(&H, a.vx, a.vy, a.xv, a.yv, a.e, a.nx, a.ny); };
        CASE("valid", )
        CASE("Vy NULL", a.vy = nullptr)
        CASE("yv NULL", a.yv = nullptr)
        CASE("nx = 0", a.nx = 0)
        CASE("box at 2^31", a.nx = 65534; a.ny = 32766)
        CASE("Vx and Vy overlap", a.vy = A(0, 8 * ((NX + 1) * (NY + 2) - 1)))
        CASE("edge: Vy right behind Vx", a.vy = A(0, 8 * (NX + 1) * (NY + 2)))
        CASE("Vy overlaps xv", a.xv = A(1, 8))
        CASE("Vx overlaps yv", a.yv = A(0, -8 * NY))
        CASE("edge: yv right ahead of Vx", a.yv = A(0, -8 * (NY + 1)))
    }
    {
        g_entry = "jrx_pureshear_bc3d";
        struct { double *v[3]; const double *x[3]; double e; int64_t nx, ny, nz; } good = {{A(0), A(1), A(2)}, {A(3), A(4), A(5)}, 1.0, NX, NY, NZ};
        auto call = [](auto &a) { return jrx_pureshear_bc3d(&H, a.v[0], a.v[1], a.v[2], a.x[0], a.x[1], a.x[2], a.e, a.nx, a.ny, a.nz); };
        CASE("valid", )
        CASE("Vz NULL", a.v[2] = nullptr)
        CASE("xv NULL", a.x[0] = nullptr)
        CASE("nz = 0", a.nz = 0)
        CASE("box at 2^31", a.nx = 2046; a.ny = 1022; a.nz = 1022)
        CASE("Vy and Vz overlap", a.v[2] = A(1, 8))
        CASE("Vz overlaps xv", a.x[0] = A(2, 8))
        CASE("edge: zv right behind Vz", a.x[2] = A(2, 8 * (NX + 2) * (NY + 2) * (NZ + 1)))
    }
    {
        g_entry = "jrx_free_surface_bcs2d";
        struct { const double *vx; double *vy; const double *c[4], *ph; const jrx_rheology *rh; double dt, dx, dy; const double *dxi, *dyj; int64_t nx, ny;
                 int32_t on; } good = {A(0), A(1), {A(2), A(3), A(4), A(5)}, A(6), &rh, 0.5, 0.2, 0.25, nullptr, nullptr, NX, NY, 1};
        auto call = [](auto &a) {
            return jrx_free_surface_bcs2d(&H, a.vx, a.vy, a.c[0], a.c[1], a.c[2], a.c[3], a.ph, a.rh, a.dt, a.dx, a.dy, a.dxi, a.dyj, a.nx, a.ny, a.on);
        };
        CASE("valid", )
        CASE("off: nothing is looked at", a.on = 0; a.vy = nullptr)
        CASE("P0 NULL", a.c[1] = nullptr)
        CASE("rheology NULL", a.rh = nullptr)
        CASE("ny = 0", a.ny = 0)
        CASE("0 phases", a.rh = &rh0)
        CASE("9 phases", a.rh = &rh9)
        CASE("box at 2^31", a.nx = 65534; a.ny = 32766)
        CASE("the phase ratios at 2^31", a.nx = 32768; a.ny = 32768)
        CASE("dt = 0", a.dt = 0.0)
        CASE("dt Inf", a.dt = kInf)
        CASE("dx NaN", a.dx = kNaN)
        CASE("valid: dx NaN with a spacing array", a.dx = kNaN; a.dxi = A(7))
        CASE("dy = -1 with dx_i alone", a.dy = -1.0; a.dxi = A(7))
        CASE("Vy overlaps η", a.c[3] = A(1, 8))
        CASE("Vy overlaps Vx", a.vx = A(1, 8))
        CASE("Vy overlaps the phase ratios", a.ph = A(1, -8 * (2 * NX * NY - 1)))
        CASE("edge: the phase ratios right ahead of Vy", a.ph = A(1, -8 * 2 * NX * NY))
    }
    {
        g_entry = "jrx_free_surface_bcs3d";
        struct { const double *vx, *vy; double *vz; const double *c[4], *ph; const jrx_rheology *rh; double dt, dx, dy, dz; int64_t nx, ny, nz; int32_t on; } good = {
            A(0), A(1), A(2), {A(3), A(4), A(5), A(6)}, A(7), &rh, 0.5, 0.2, 0.25, 0.3, NX, NY, NZ, 1};
        auto call = [](auto &a) {
            return jrx_free_surface_bcs3d(&H, a.vx, a.vy, a.vz, a.c[0], a.c[1], a.c[2], a.c[3], a.ph, a.rh, a.dt, a.dx, a.dy, a.dz, a.nx, a.ny, a.nz, a.on);
        };
        CASE("valid", )
        CASE("off: nothing is looked at", a.on = 0; a.vz = nullptr)
        CASE("Vz NULL", a.vz = nullptr)
        CASE("phase ratios NULL", a.ph = nullptr)
        CASE("nx = 0", a.nx = 0)
        CASE("9 phases", a.rh = &rh9)
        CASE("box at 2^31", a.nx = 2046; a.ny = 1022; a.nz = 1022)
        CASE("dt NaN", a.dt = kNaN)
        CASE("dz = 0", a.dz = 0.0)
        CASE("Vz overlaps Vy", a.vy = A(2, 8))
        CASE("Vz overlaps P", a.c[0] = A(2, 8))
        CASE("Vz overlaps the phase ratios", a.ph = A(2, 8))
    }
    jrx_thermal_phases tp = {};
    tp.nphase = 2;
    jrx_thermal_phases tp0 = tp;
    tp0.nphase = 0;
    static const int64_t n3[3] = {NX, NY, NZ}, n0[3] = {NX, 0, NZ}, nbox2[3] = {65534, 32766, 1}, nbox3[3] = {2046, 1022, 1022}, nph[3] = {32768, 32768, 1};
    static const double di[3] = {0.2, 0.25, 0.3}, dibad[3] = {0.2, 0.0, 0.3}, dibad3[3] = {0.2, 0.25, kInf};
    {
        g_entry = "jrx_subgrid_characteristic_time";
        struct { double *dt0; const double *ph; const jrx_thermal_phases *tp; const double *T, *P; const int64_t *n; int32_t nd; const double *di; } good = {
            A(0), A(1), &tp, A(2), A(3), n3, 3, di};
        auto call = [](auto &a) { return jrx_subgrid_characteristic_time(&H, a.dt0, a.ph, a.tp, a.T, a.P, a.n, a.nd, a.di); };
        CASE("valid 3D", )
        CASE("valid 2D", a.nd = 2)
        CASE("T NULL", a.T = nullptr)
        CASE("di NULL", a.di = nullptr)
        CASE("ndim = 4", a.nd = 4)
        CASE("0 phases", a.tp = &tp0)
        CASE("ny = 0", a.n = n0)
        CASE("2D box at 2^31", a.nd = 2; a.n = nbox2)
        CASE("3D box at 2^31", a.n = nbox3)
        CASE("the phase ratios at 2^31", a.nd = 2; a.n = nph)
        CASE("di[2] = 0", a.di = dibad)
        CASE("2D: di[3] is not read", a.nd = 2; a.di = dibad3)
        CASE("di[3] Inf", a.di = dibad3)
        CASE("dt₀ overlaps T", a.T = A(0, 8))
        CASE("dt₀ overlaps P", a.P = A(0, 8 * (NX * NY * NZ - 1)))
        CASE("edge: P right behind dt₀", a.P = A(0, 8 * NX * NY * NZ))
        CASE("dt₀ overlaps the phase ratios", a.ph = A(0, -8 * (2 * NX * NY * NZ - 1)))
        CASE("edge: 2D, T (ni .+ 2, no third axis) right ahead of dt₀", a.nd = 2; a.T = A(0, -8 * (NX + 2) * (NY + 2)))
    }
    jrx_melting ml = {};
    ml.nphase = 2, ml.kind[1] = 1;
    jrx_melting ml9 = ml, mlk = ml;
    ml9.nphase = 9, mlk.kind[0] = 2;
    static const int64_t nbelow[3] = {k2G - 1, 1, 1}, nat[3] = {k2G / 2, 2, 1}, nhalf[3] = {k2G / 2, 1, 1};
    {
        g_entry = "jrx_compute_melt_fraction";
        struct { double *phi; const double *ph; const jrx_melting *m; const double *T; double Ts; const double *P; double Ps; const int64_t *n; int32_t nd; } good = {
            A(0), A(1), &ml, A(2), 0.0, A(3), 0.0, n3, 3};
        auto call = [](auto &a) { return jrx_compute_melt_fraction(&H, a.phi, a.ph, a.m, a.T, a.Ts, a.P, a.Ps, a.n, a.nd); };
        CASE("valid 3D", )
        CASE("valid 2D", a.nd = 2)
        CASE("valid: T, P and the phase ratios absent", a.T = nullptr; a.P = nullptr; a.ph = nullptr)
        CASE("valid: T absent", a.T = nullptr)
        CASE("ϕ NULL", a.phi = nullptr)
        CASE("n NULL", a.n = nullptr)
        CASE("ndim = 1", a.nd = 1)
        CASE("9 phases", a.m = &ml9)
        CASE("melting kind 2", a.m = &mlk)
        CASE("ny = 0", a.n = n0)
        CASE("edge: one below 2^31 cells, no phase ratios", a.ph = nullptr; a.n = nbelow)
        CASE("edge: 2^31 cells, no phase ratios", a.ph = nullptr; a.n = nat)
        CASE("edge: 2^30 cells, two phases", a.n = nhalf)
        CASE("ϕ overlaps T", a.T = A(0, 8))
        CASE("ϕ overlaps P", a.P = A(0, 8))
        CASE("ϕ overlaps the phase ratios", a.ph = A(0, 8 * (NX * NY * NZ - 1)))
        CASE("edge: the phase ratios right behind ϕ", a.ph = A(0, 8 * NX * NY * NZ))
    }
}

// ------------------------------------------------------------------------------------------------ gridops.hip
void gridops()
{
    {
        g_entry = "jrx_velocity2vertex2d";
        struct { double *o[2]; const double *v[2]; int64_t nx, ny, mx, my; } good = {{A(0), A(1)}, {A(2), A(3)}, NX, NY, NX + 1, NY + 1};
        auto call = [](auto &a) { return jrx_velocity2vertex2d(&H, a.o[0], a.o[1], a.v[0], a.v[1], a.nx, a.ny, a.mx, a.my); };
        CASE("valid", )
        CASE("valid: smaller outputs", a.mx = 1; a.my = 1)
        CASE("Vy_v NULL", a.o[1] = nullptr)
        CASE("Vx NULL", a.v[0] = nullptr)
        CASE("ny = 0", a.ny = 0)
        CASE("mx = 0", a.mx = 0)
        CASE("my = ny + 2", a.my = NY + 2)
    }
    {
        g_entry = "jrx_velocity2vertex3d";
        struct { double *o[3]; const double *v[3]; int64_t nx, ny, nz, mx, my, mz; } good = {{A(0), A(1), A(2)}, {A(3), A(4), A(5)}, NX, NY, NZ, NX + 1, NY + 1, NZ + 1};
        auto call = [](auto &a) { return jrx_velocity2vertex3d(&H, a.o[0], a.o[1], a.o[2], a.v[0], a.v[1], a.v[2], a.nx, a.ny, a.nz, a.mx, a.my, a.mz); };
        CASE("valid", )
        CASE("Vz_v NULL", a.o[2] = nullptr)
        CASE("Vz NULL", a.v[2] = nullptr)
        CASE("nz = 0", a.nz = 0)
        CASE("mz = 0", a.mz = 0)
        CASE("mz = nz + 2", a.mz = NZ + 2)
        CASE("mx = nx + 2", a.mx = NX + 2)
    }
    {
        g_entry = "jrx_velocity2center2d";
        struct { double *o[2]; const double *v[2]; int64_t nx, ny; } good = {{A(0), A(1)}, {A(2), A(3)}, NX, NY};
        auto call = [](auto &a) { return jrx_velocity2center2d(&H, a.o[0], a.o[1], a.v[0], a.v[1], a.nx, a.ny); };
        CASE("valid", )
        CASE("Vx_c NULL", a.o[0] = nullptr)
        CASE("Vy NULL", a.v[1] = nullptr)
        CASE("nx = 0", a.nx = 0)
    }
    {
        g_entry = "jrx_velocity2center3d";
        struct { double *o[3]; const double *v[3]; int64_t nx, ny, nz; } good = {{A(0), A(1), A(2)}, {A(3), A(4), A(5)}, NX, NY, NZ};
        auto call = [](auto &a) { return jrx_velocity2center3d(&H, a.o[0], a.o[1], a.o[2], a.v[0], a.v[1], a.v[2], a.nx, a.ny, a.nz); };
        CASE("valid", )
        CASE("Vz_c NULL", a.o[2] = nullptr)
        CASE("Vx NULL", a.v[0] = nullptr)
        CASE("nz = 0", a.nz = 0)
    }
    static const int64_t vd[3] = {NX + 1, NY + 1, NZ + 1}, cd[3] = {NX, NY, NZ}, cdg[3] = {NX + 1, NY, NZ}, vd1[3] = {NX + 1, 1, NZ + 1}, cdz[3] = {NX, NY, NZ - 1};
    {
        g_entry = "jrx_vertex2center";
        struct { double *c; const double *v; const int64_t *vd, *cd; int32_t nd, gx, gy, gz; } good = {A(0), A(1), vd, cd, 3, 0, 0, 0};
        auto call = [](auto &a) { return jrx_vertex2center(&H, a.c, a.v, a.vd, a.cd, a.nd, a.gx, a.gy, a.gz); };
        CASE("valid 3D", )
        CASE("valid 2D", a.nd = 2)
        CASE("valid: a ghost layer along x", a.gx = 1; a.cd = cdg)
        CASE("center NULL", a.c = nullptr)
        CASE("cdim NULL", a.cd = nullptr)
        CASE("ndim = 1", a.nd = 1)
        CASE("a ghost layer along x, centre array without it", a.gx = 1)
        CASE("one vertex along y", a.vd = vd1)
        CASE("centre array too small along z", a.cd = cdz)
        CASE("2D: the third axis is not read", a.nd = 2; a.cd = cdz; a.gz = 1)
    }
    {
        g_entry = "jrx_center2vertex_harm2d";
        struct { double *v; const double *c; int64_t nx, ny; } good = {A(0), A(1), NX, NY};
        auto call = [](auto &a) { return jrx_center2vertex_harm2d(&H, a.v, a.c, a.nx, a.ny); };
        CASE("valid", )
        CASE("vertex NULL", a.v = nullptr)
        CASE("center NULL", a.c = nullptr)
        CASE("ny = 0", a.ny = 0)
    }
    {
        g_entry = "jrx_center2vertex3d";
        struct { double *v[3]; const double *c[3]; int64_t nx, ny, nz; } good = {{A(0), A(1), A(2)}, {A(3), A(4), A(5)}, NX, NY, NZ};
        auto call = [](auto &a) { return jrx_center2vertex3d(&H, a.v[0], a.v[1], a.v[2], a.c[0], a.c[1], a.c[2], a.nx, a.ny, a.nz); };
        CASE("valid", )
        CASE("vertex_xy NULL", a.v[2] = nullptr)
        CASE("center_yz NULL", a.c[0] = nullptr)
        CASE("nx = 0", a.nx = 0)
    }
    jrx_rheology rh = {};
    rh.nphase = 2, rh.has_density = 1;
    jrx_rheology rh0 = rh, rh9 = rh, rhnd = rh, rhpl = rh;
    rh0.nphase = 0, rh9.nphase = 9, rhnd.has_density = 0, rhpl.visc_kind[0] = 2;
    static const int64_t n3[3] = {NX, NY, NZ}, n0[3] = {NX, NY, 0}, tg[3] = {NX + 2, NY + 2, NZ + 2}, tsmall[3] = {NX, NY - 1, NZ}, tmixed[3] = {NX + 2, NY, NZ + 2};
    {
        g_entry = "jrx_compute_rhog";
        struct { double *rhog; const jrx_rheology *rh; const double *ph, *T, *P; const int64_t *n, *td; int32_t nd; } good = {A(0), &rh, A(1), A(2), A(3), n3, tg, 3};
        auto call = [](auto &a) { return jrx_compute_rhog(&H, a.rhog, a.rh, a.ph, a.T, a.P, a.n, a.td, a.nd); };
        CASE("valid 3D", )
        CASE("valid 2D, no phase ratios, no tdim", a.nd = 2; a.ph = nullptr; a.td = nullptr)
        CASE("ρg NULL", a.rhog = nullptr)
        CASE("rheology NULL", a.rh = nullptr)
        CASE("ndim = 4", a.nd = 4)
        CASE("0 phases", a.rh = &rh0)
        CASE("9 phases", a.rh = &rh9)
        CASE("no density law", a.rh = &rhnd)
        CASE("nz = 0", a.n = n0)
        CASE("args.T smaller along 2", a.td = tsmall)
    }
    static const int64_t nneg[3] = {NX, -1, NZ};
    {
        g_entry = "jrx_compute_lithostatic_pressure";
        struct { double *P; const double *rhog; double dz; const double *dzc; const int64_t *n; int32_t nd; } good = {A(0), A(1), 0.25, nullptr, n3, 3};
        auto call = [](auto &a) { return jrx_compute_lithostatic_pressure(&H, a.P, a.rhog, a.dz, a.dzc, a.n, a.nd); };
        CASE("valid 3D", )
        CASE("valid 2D", a.nd = 2)
        CASE("P NULL", a.P = nullptr)
        CASE("n NULL", a.n = nullptr)
        CASE("ndim = 0", a.nd = 0)
        CASE("ny = -1", a.n = nneg)
        CASE("2D: n[2] is not read", a.nd = 2; a.n = n0)
        g_comm = true;
        CASE("the vertical direction split across ranks", )
        g_comm = false;
    }
    {
        g_entry = "jrx_compute_viscosity_single";
        struct { double *eta; const jrx_rheology *rh; const double *T, *P; const int64_t *n, *td; int32_t nd; double nu, lo, hi; const double *AII; int32_t tf; } good = {
            A(0), &rh, A(1), A(2), n3, tg, 3, 1.0, 1e16, 1e24, nullptr, 0};
        auto call = [](auto &a) { return jrx_compute_viscosity_single(&H, a.eta, a.rh, a.T, a.P, a.n, a.td, a.nd, a.nu, a.lo, a.hi, a.AII, a.tf); };
        CASE("valid: ghosted T", )
        CASE("valid: T at the cell centres", a.td = n3)
        CASE("valid: no T", a.T = nullptr; a.td = tmixed)
        CASE("η NULL", a.eta = nullptr)
        CASE("ndim = 5", a.nd = 5)
        CASE("0 phases", a.rh = &rh0)
        CASE("nz = 0", a.n = n0)
        CASE("args.T neither ni nor ni .+ 2", a.td = tmixed)
        CASE("power-law creep without the invariant", a.rh = &rhpl)
        CASE("valid: power-law creep with the invariant", a.rh = &rhpl; a.AII = A(3))
    }
    {
        g_entry = "jrx_compute_shear_heating";
        static const double chi[JRX_MAXPHASE] = {};
        const double *t[6] = {A(1), A(2), A(3), A(4), A(5), A(6)}, *to[6] = {A(7), A(8), A(9), A(10), A(11), A(12)}, *e[6] = {A(13), A(14), A(15), A(16), A(17), A(18)};
        const double *tn[6] = {A(1), A(2), A(3), nullptr, A(5), A(6)}, *en[6] = {A(13), A(14), nullptr, A(16), A(17), A(18)};
        struct { double *sh; const double *const *t, *const *to, *const *e; const double *ph; const jrx_rheology *rh; const double *chi; double dt; const int64_t *n;
                 int32_t nd; } good = {A(0), t, to, e, A(19), &rh, chi, 0.5, n3, 3};
        auto call = [](auto &a) { return jrx_compute_shear_heating(&H, a.sh, a.t, a.to, a.e, a.ph, a.rh, a.chi, a.dt, a.n, a.nd); };
        CASE("valid 3D", )
        CASE("valid 2D", a.nd = 2)
        CASE("the output NULL", a.sh = nullptr)
        CASE("τ_o NULL", a.to = nullptr)
        CASE("χ NULL", a.chi = nullptr)
        CASE("ndim = 1", a.nd = 1)
        CASE("9 phases", a.rh = &rh9)
        CASE("nz = 0", a.n = n0)
        CASE("3D: τ component 3 NULL", a.t = tn)
        CASE("valid 2D: component 3 is not read", a.nd = 2; a.t = tn)
        CASE("ε component 2 NULL", a.nd = 2; a.e = en)
    }
}

// ------------------------------------------------------------------------------------------------ phase_ratios.hip
void phase_ratios()
{
    const double *pa[3] = {A(10), A(11), A(12)}, *pan[3] = {A(10), A(11), nullptr};
    const double *xc[3] = {A(13), A(14), A(15)}, *xv[3] = {A(16), A(17), A(18)}, *xcn[3] = {A(13), nullptr, A(15)}, *xvn[3] = {A(16), A(17), nullptr};
    static const double dx[3] = {0.2, 0.25, 0.3}, dx0[3] = {0.2, 0.0, 0.3}, dxi[3] = {0.2, 0.25, kInf};
    {
        g_entry = "jrx_update_phase_ratios2d";
        H.phase_ratios_fused = true;
        struct { double *c, *v, *vx, *vy; const double *const *pa; int32_t np; int64_t nx, ny; const double *const *xc, *const *xv; const double *dx; } good = {
            A(0), A(1), A(2), A(3), pa, 3, NX, NY, xc, xv, dx};
        auto call = [](auto &a) { return jrx_update_phase_ratios2d(&H, a.c, a.v, a.vx, a.vy, a.pa, a.np, a.nx, a.ny, a.xc, a.xv, a.dx); };
        const double *paov[3] = {A(10), A(11), A(3, 8)}, *xcov[3] = {A(13), A(1, 8 * (3 * (NX + 1) * (NY + 1) - 1)), A(15)}, *xvadj[3] = {A(16), A(0, -8 * (NY + 1)), A(18)};
        CASE("valid", )
        CASE("the phase arrays NULL", a.pa = nullptr)
        CASE("dx NULL", a.dx = nullptr)
        CASE("vertex NULL", a.v = nullptr)
        CASE("Vy NULL", a.vy = nullptr)
        CASE("nphase = 0", a.np = 0)
        CASE("nphase = 9", a.np = 9)
        CASE("phase array 3 NULL", a.pa = pan)
        CASE("valid: two phases, the third array is not read", a.pa = pan; a.np = 2)
        CASE("xc[2] NULL", a.xc = xcn)
        CASE("valid: the third coordinate vector is not read", a.xv = xvn)
        CASE("ny = 0", a.ny = 0)
        CASE("dx[2] = 0", a.dx = dx0)
        CASE("valid: dx[3] is not read", a.dx = dxi)
        CASE("vertex at 2^31 entries", a.np = 2; a.nx = 32767; a.ny = 32767)
        CASE("center and Vy overlap", a.vy = A(0, 8))
        CASE("Vy overlaps phase array 3", a.pa = paov)
        CASE("vertex overlaps xc[2]", a.xc = xcov)
        CASE("edge: xv[2] right ahead of center", a.xv = xvadj)
        CASE("edge: vertex right behind center", a.v = A(0, 8 * 3 * NX * NY))
        CASE("edge: vertex starts on the last entry of center", a.v = A(0, 8 * (3 * NX * NY - 1)))
    }
    {
        g_entry = "jrx_update_phase_ratios3d";
        struct { double *o[8]; const double *const *pa; int32_t np; int64_t nx, ny, nz; const double *const *xc, *const *xv; const double *dx; } good = {
            {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7)}, pa, 3, NX, NY, NZ, xc, xv, dx};
        auto call = [](auto &a) {
            return jrx_update_phase_ratios3d(&H, a.o[0], a.o[1], a.o[2], a.o[3], a.o[4], a.o[5], a.o[6], a.o[7], a.pa, a.np, a.nx, a.ny, a.nz, a.xc, a.xv, a.dx);
        };
        const double *paov[3] = {A(5, 8), A(11), A(12)}, *xvov[3] = {A(16), A(17), A(7, -8 * NZ)};
        CASE("valid", )
        CASE("xv NULL", a.xv = nullptr)
        CASE("yz NULL", a.o[5] = nullptr)
        CASE("nphase = 0", a.np = 0)
        CASE("phase array 3 NULL", a.pa = pan)
        CASE("xv[3] NULL", a.xv = xvn)
        CASE("nz = 0", a.nz = 0)
        CASE("dx[3] Inf", a.dx = dxi)
        CASE("vertex at 2^31 entries", a.np = 2; a.nx = 1023; a.ny = 1023; a.nz = 1023)
        CASE("vertex and xz overlap", a.o[6] = A(1, 8))
        CASE("yz overlaps phase array 1", a.pa = paov)
        CASE("xy overlaps xv[3]", a.xv = xvov)
    }
}

// ------------------------------------------------------------------------------------------------ stress_rotation.hip
void stress_rotation()
{
    static const double idi[3] = {5.0, 4.0, 3.0};
    {
        g_entry = "jrx_rotate_stress2d";
        double *to[6] = {A(0), A(1), A(2), A(3), A(4), A(5)};
        const double *t[6] = {A(6), A(7), A(8), A(9), A(10), A(11)}, *V[2] = {A(13), A(14)};
        struct { double *const *to; const double *const *t; const double *w; const double *const *V; int64_t nx, ny; const double *idi; double dt; int32_t m, adv; } good = {
            to, t, A(12), V, NX, NY, idi, 0.1, JRX_ROTATE_MATRIX, JRX_ADVECT_UPWIND};
        auto call = [](auto &a) { return jrx_rotate_stress2d(&H, a.to, a.t, a.w, a.V, a.nx, a.ny, a.idi, a.dt, a.m, a.adv); };
        double *to4[6] = {A(0), A(1), A(2), A(3), nullptr, nullptr}, *ton[6] = {A(0), A(1), nullptr, A(3), A(4), A(5)}, *toin[6] = {A(0), A(8, 8), A(2), A(3), A(4), A(5)};
        double *toout[6] = {A(0), A(1), A(2), A(3), A(4), A(3, 8)}, *tov[6] = {A(0), A(1), A(2), A(14, 8), A(4), A(5)}, *tow[6] = {A(0), A(1), A(12), A(3), A(4), A(5)};
        double *toadj[6] = {A(0), A(0, 8 * NX * NY), A(2), A(3), A(4), A(5)}, *tolast[6] = {A(0), A(0, 8 * (NX * NY - 1)), A(2), A(3), A(4), A(5)};
        const double *tn[6] = {A(6), nullptr, A(8), A(9), A(10), A(11)}, *t5[6] = {A(6), A(7), A(8), A(9), A(10), nullptr}, *Vn[2] = {A(13), nullptr};
        CASE("valid", )
        CASE("valid: no vertex normals (τ_o.xx_v, τ_o.yy_v absent)", a.to = to4)
        CASE("valid: no vertex normals (τ.yy_v absent): τ_o.xx_v and τ_o.yy_v are not looked at", a.t = t5; a.to = toout)
        CASE("valid: no advection, no velocities", a.adv = JRX_ADVECT_NONE; a.V = nullptr)
        CASE("τ_o NULL", a.to = nullptr)
        CASE("_di NULL", a.idi = nullptr)
        CASE("method = 2", a.m = 2)
        CASE("advection = 2", a.adv = 2)
        CASE("nx = 0", a.nx = 0)
        CASE("box at 2^31", a.nx = 65534; a.ny = 32766)
        CASE("V NULL with advection", a.V = nullptr)
        CASE("τ.yy NULL", a.t = tn)
        CASE("τ_o.xy_c NULL", a.to = ton)
        CASE("ω.xy NULL", a.w = nullptr)
        CASE("V.Vy NULL", a.V = Vn)
        CASE("τ_o.yy overlaps τ.xy_c", a.to = toin)
        CASE("τ_o.xy_c overlaps ω.xy", a.to = tow)
        CASE("τ_o.xy overlaps V.Vy", a.to = tov)
        CASE("valid: τ_o.xy on V.Vy without advection", a.to = tov; a.adv = JRX_ADVECT_NONE)
        CASE("τ_o.xy and τ_o.yy_v overlap", a.to = toout)
        CASE("edge: τ_o.yy right behind τ_o.xx", a.to = toadj)
        CASE("edge: τ_o.yy starts on the last entry of τ_o.xx", a.to = tolast)
    }
    {
        g_entry = "jrx_rotate_stress3d";
        double *to[9] = {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7), A(8)};
        const double *t[9] = {A(10), A(11), A(12), A(13), A(14), A(15), A(16), A(17), A(18)}, *w[3] = {A(20), A(21), A(22)}, *V[3] = {A(23), A(24), A(25)};
        struct { double *const *to; const double *const *t, *const *w, *const *V; int64_t nx, ny, nz; const double *idi; double dt; int32_t m, adv; } good = {
            to, t, w, V, NX, NY, NZ, idi, 0.1, JRX_ROTATE_JAUMANN, JRX_ADVECT_UPWIND};
        auto call = [](auto &a) { return jrx_rotate_stress3d(&H, a.to, a.t, a.w, a.V, a.nx, a.ny, a.nz, a.idi, a.dt, a.m, a.adv); };
        double *ton[9] = {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7), nullptr}, *toin[9] = {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(7), A(21, 8)};
        double *toout[9] = {A(0), A(1), A(2), A(3), A(4), A(5), A(6), A(0, 8), A(8)}, *tov[9] = {A(23, -8 * (NX * NY * NZ - 1)), A(1), A(2), A(3), A(4), A(5), A(6), A(7), A(8)};
        double *toadj[9] = {A(23, -8 * NX * NY * NZ), A(1), A(2), A(3), A(4), A(5), A(6), A(7), A(8)};
        const double *tn[9] = {A(10), A(11), A(12), A(13), A(14), A(15), nullptr, A(17), A(18)}, *wn[3] = {A(20), nullptr, A(22)}, *Vn[3] = {nullptr, A(24), A(25)};
        CASE("valid", )
        CASE("valid: no advection, the velocities absent", a.adv = JRX_ADVECT_NONE; a.V = Vn)
        CASE("ω NULL", a.w = nullptr)
        CASE("method = -1", a.m = -1)
        CASE("advection = -1", a.adv = -1)
        CASE("nz = 0", a.nz = 0)
        CASE("box at 2^31", a.nx = 2046; a.ny = 1022; a.nz = 1022)
        CASE("V NULL with advection", a.V = nullptr)
        CASE("τ.yz NULL", a.t = tn)
        CASE("τ_o.xy NULL", a.to = ton)
        CASE("ω.xz NULL", a.w = wn)
        CASE("V.Vx NULL", a.V = Vn)
        CASE("τ_o.xy overlaps ω.xz", a.to = toin)
        CASE("τ_o.xx overlaps V.Vx", a.to = tov)
        CASE("edge: τ_o.xx right ahead of V.Vx", a.to = toadj)
        CASE("τ_o.xx and τ_o.xz overlap", a.to = toout)
    }
}

// ------------------------------------------------------------------------------------------------ particles.hip, particles3d.hip: the checks that stand on op_args.hpp
void particles()
{
    const int64_t ns = NX * NY * 6, ns3 = NX * NY * NZ * 6;          // slots: max_xcell = 6
    {
        g_entry = "jrx_particles2d_grid2particle";
        const jrx_particles2d P = {A(0), A(1), (int32_t *)A(2), NX, NY, 6, 0.0, 0.0, 0.5, 0.25, 2.0, 4.0};
        struct { double *pF; const double *F; const jrx_particles2d *P; } good = {A(3), A(4), &P};
        auto call = [](auto &a) { return jrx_particles2d_grid2particle(&H, a.pF, a.F, a.P); };
        CASE("valid", )
        CASE("particles NULL", a.P = nullptr)
        CASE("pF NULL", a.pF = nullptr)
        CASE("F NULL", a.F = nullptr)
        CASE("pF overlaps py", a.pF = A(1, 8 * (ns - 1)))
        CASE("edge: pF right behind py", a.pF = A(1, 8 * ns))
        CASE("pF overlaps the mask", a.pF = A(2, -8 * ns + 4))
        CASE("edge: pF right ahead of the mask", a.pF = A(2, -8 * ns))
        CASE("edge: pF right behind the mask (4-byte entries)", a.pF = A(2, 4 * ns))
        CASE("pF overlaps F", a.F = A(3, 8 * (ns - 1)))
        CASE("edge: F right behind pF", a.F = A(3, 8 * ns))
        g_comm = true;
        CASE("a handle with a communicator", )
        g_comm = false;
    }
    {
        g_entry = "jrx_particles2d_phase_ratios";
        const jrx_particles2d P = {A(0), A(1), (int32_t *)A(2), NX, NY, 6, 0.0, 0.0, 0.5, 0.25, 2.0, 4.0};
        int64_t n_empty = 0;
        struct { double *c, *v, *vx, *vy; const double *pp; int32_t np; const jrx_particles2d *P; int64_t *ne; } good = {A(3), A(4), A(5), A(6), A(7), 2, &P, &n_empty};
        auto call = [](auto &a) { return jrx_particles2d_phase_ratios(&H, a.c, a.v, a.vx, a.vy, a.pp, a.np, a.P, a.ne); };
        CASE("valid", )
        CASE("vertex NULL", a.v = nullptr)
        CASE("pPhases NULL", a.pp = nullptr)
        CASE("n_empty NULL", a.ne = nullptr)
        CASE("nphase = 9", a.np = 9)
        CASE("center and Vy overlap", a.vy = A(3, 8 * (2 * NX * NY - 1)))
        CASE("edge: Vy right behind center", a.vy = A(3, 8 * 2 * NX * NY))
        CASE("vertex overlaps pPhases", a.pp = A(4, 8))
        CASE("Vx overlaps px", a.vx = A(0, 8))
    }
    {
        g_entry = "jrx_particles2d_move";
        const jrx_particles2d S = {A(0), A(1), (int32_t *)A(2), NX, NY, 6, 0.0, 0.0, 0.5, 0.25, 2.0, 4.0};
        const jrx_particles2d D = {A(3), A(4), (int32_t *)A(5), NX, NY, 6, 0.0, 0.0, 0.5, 0.25, 2.0, 4.0};
        jrx_particles2d Dpx = D, Dact = D;
        Dpx.py = A(3, 8), Dact.active = (int32_t *)A(1, 8);
        const double *as[2] = {A(6), A(7)};
        double *ad[2] = {A(8), A(9)}, *adsrc[2] = {A(8), A(6, 8)}, *adtwo[2] = {A(8), A(8, 8 * (ns - 1))};
        int64_t counts[5] = {};
        struct { const jrx_particles2d *S, *D; const double *const *as; double *const *ad; int32_t na; int64_t *counts; } good = {&S, &D, as, ad, 2, counts};
        auto call = [](auto &a) { return jrx_particles2d_move(&H, a.S, a.D, a.as, a.ad, a.na, a.counts); };
        CASE("valid", )
        CASE("counts NULL", a.counts = nullptr)
        CASE("two arrays of the destination overlap: px and py", a.D = &Dpx)
        CASE("the destination's mask on the source's py", a.D = &Dact)
        CASE("a destination field on a source field", a.ad = adsrc)
        CASE("two destination fields overlap", a.ad = adtwo)
    }
    {
        g_entry = "jrx_particles3d_grid2particle";
        const jrx_particles3d P = {A(0), A(1), A(2), (int32_t *)A(3), NX, NY, NZ, 6, 0.0, 0.0, 0.0, 0.5, 0.25, 0.125, 2.0, 4.0, 8.0};
        struct { double *pF; const double *F; const jrx_particles3d *P; } good = {A(4), A(5), &P};
        auto call = [](auto &a) { return jrx_particles3d_grid2particle(&H, a.pF, a.F, a.P); };
        CASE("valid", )
        CASE("pF NULL", a.pF = nullptr)
        CASE("pF overlaps pz", a.pF = A(2, 8 * (ns3 - 1)))
        CASE("edge: pF right behind pz", a.pF = A(2, 8 * ns3))
        CASE("pF overlaps F", a.F = A(4, -8 * ((NX + 1) * (NY + 1) * (NZ + 1) - 1)))
        CASE("edge: F right ahead of pF", a.F = A(4, -8 * (NX + 1) * (NY + 1) * (NZ + 1)))
    }
    {
        g_entry = "jrx_particles3d_phase_ratios";
        const jrx_particles3d P = {A(0), A(1), A(2), (int32_t *)A(3), NX, NY, NZ, 6, 0.0, 0.0, 0.0, 0.5, 0.25, 0.125, 2.0, 4.0, 8.0};
        double *m[8] = {A(10), A(11), A(12), A(13), A(14), A(15), A(16), A(17)}, *mn[8] = {A(10), A(11), A(12), nullptr, A(14), A(15), A(16), A(17)};
        double *mtwo[8] = {A(10), A(11), A(12), A(13), A(14), A(15), A(16), A(11, 8)}, *mpx[8] = {A(10), A(11), A(0, 8), A(13), A(14), A(15), A(16), A(17)};
        int64_t n_empty = 0;
        struct { double *const *m; const double *pp; int32_t np; const jrx_particles3d *P; int64_t *ne; } good = {m, A(18), 2, &P, &n_empty};
        auto call = [](auto &a) { return jrx_particles3d_phase_ratios(&H, a.m, a.pp, a.np, a.P, a.ne); };
        CASE("valid", )
        CASE("phase_ratios NULL", a.m = nullptr)
        CASE("member 4 NULL", a.m = mn)
        CASE("pPhases NULL", a.pp = nullptr)
        CASE("two members overlap", a.m = mtwo)
        CASE("a member overlaps px", a.m = mpx)
        CASE("a member overlaps pPhases", a.pp = A(17, 8))
    }
}

}  // namespace

int main()
{
    topography();
    advection();
    principal();
    stepops();
    gridops();
    phase_ratios();
    stress_rotation();
    particles();
    fprintf(stderr, "%d scenarios\n", g_lines);
    return 0;
}
