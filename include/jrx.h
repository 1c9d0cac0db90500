/*
 * jrx.h -- C ABI of the MI355X-native pseudo-transient (PT) Stokes / heat-diffusion hot path.
 *
 * This is the drop-in boundary for JustRelax.jl's backend method table: a Julia extension
 * defines solve!(::Trait, stokes, ...), heatdiffusion_PT!(::Trait, thermal, ...), flow_bcs!,
 * thermal_bcs!, velocity2displacement!, compute_maxloc! for its trait and forwards each to one
 * entry point below with `ccall`, passing `pointer(A)` of its ROCArray{Float64} fields
 * (INTEGRATION.md shows the shim).  Reference seam being replaced:
 *   src/ext/AMDGPU/3D.jl:397-407, src/ext/AMDGPU/2D.jl (forwarding methods onto _solve!),
 *   src/stokes/Stokes3D.jl:18-23, src/stokes/Stokes2D.jl:12-17,
 *   src/thermal_diffusion/DiffusionPT_solver.jl:11-17.
 * All file:line citations are relative to the reference checkout (PTsolvers/JustRelax.jl v0.7.1).
 *
 * Conventions
 *  - every array is device memory, fp64, dense, column-major (x fastest) -- Julia's layout; the
 *    library never allocates, frees or re-lays-out a caller array (the caller keeps them alive
 *    for the duration of the call: GC.@preserve);
 *  - extents follow src/types/constructors/stokes.jl and .../heat_diffusion.jl, e.g. in 3D with
 *    ni = (nx,ny,nz): Vx (nx+1,ny+2,nz+2), txy (nx+1,ny+1,nz), Rx (nx-1,ny,nz), T (nx+2,ny+2);
 *  - calls are synchronous at the ABI (they return after the handle's stream has drained) except
 *    the *_async kernels-only entry points, which only enqueue;
 *  - every function returns a jrx_status; jrx_last_error() gives the message. Never aborts.
 *  - a handle is bound to one GPU and is not thread-safe (one handle per GPU / per rank).
 */
#ifndef JRX_H
#define JRX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JRX_VERSION 230

typedef enum jrx_status {
    JRX_OK = 0,
    JRX_ERR_NAN = 1,        /* error("NaN(s)") -- src/stokes/Stokes3D.jl:162 */
    JRX_ERR_HIP = 2,
    JRX_ERR_RCCL = 3,
    JRX_ERR_ARG = 4,
    JRX_ERR_UNSUPPORTED = 5
} jrx_status;

/* Boundary faces: one bit per face, names as in the reference's NamedTuples
 * (src/boundaryconditions/types.jl:108-157).  NOTE the reference's own 3D conventions, kept
 * verbatim: free_slip! maps `top` to k = 1 and `bot` to k = end (free_slip.jl:35-50); no_slip!
 * maps `bot` to k = 1 and `top` to k = end (no_slip.jl:44-53); periodic: bot = k = 1.
 * In 2D: bot <-> j = 1, top <-> j = end for all three. */
enum {
    JRX_FACE_LEFT = 1, JRX_FACE_RIGHT = 2, JRX_FACE_FRONT = 4, JRX_FACE_BACK = 8,
    JRX_FACE_TOP = 16, JRX_FACE_BOT = 32
};

typedef struct jrx_handle jrx_handle;

/* ------------------------------------------------------------------ lifetime */
/* Creates streams, events and reduction scratch on `device`. */
jrx_status jrx_create(int32_t device, jrx_handle **out);
jrx_status jrx_destroy(jrx_handle *h);
const char *jrx_last_error(const jrx_handle *h);   /* h may be NULL: last creation error */
int32_t jrx_version(void);
/* sha256 of the sources (csrc/ + include/jrx.h) this binary was built from; the Python binding refuses a library whose id differs from
 * the sources beside it */
const char *jrx_build_id(void);

/* ------------------------------------------------------------------ state arrays
 * Device memory for the fields, handed out by the library.  Replaces the array constructor the backend owns in the reference:
 * StokesArrays(::Type{AMDGPUBackend}, ni) / ThermalArrays(...) -> @zeros(ni...) -> ROCArray (src/ext/AMDGPU/3D.jl:46-48,
 * src/types/constructors/stokes.jl:279-303) -- a binding wraps the pointer (Julia: unsafe_wrap(ROCArray, ptr, dims; lock = false) plus a
 * finalizer that calls jrx_field_free).  Contents are NOT initialised (the constructor fills with zeros as @zeros does).  Using it is
 * optional: every entry point takes any device pointer.  What it buys: the option "field_placement" decides how the arrays are backed
 * physically, and the large 3D kernels are sensitive to that (the same launch takes 4.7 .. 6.9 ms at 512^3: DESIGN.md section 3, profiles/r05_placement_search.txt).  With
 * "field_placement" = 1 every large array is mapped ONCE, at a virtual range never used before, onto physical chunks picked at random from a pool that spans most of the free
 * memory (tuning keys "field_chunk_mib", "field_pool_pct": include/jrx_tuning.h); the library's own large arrays (second state sets, ητ) follow the same option.  An array is
 * never moved afterwards.  jrx_destroy releases whatever the caller has not freed.  jrx_field_trim returns the pool's unused chunks to the driver (call it once the arrays of a
 * run exist -- the library's second state set is made by the first driver call).  The pool is filled when a large array is requested while no array of that chunk size is live
 * (the first array of a run); arrays made later get chunks created on the spot.
 * jrx_field_stats: [0] live arrays (the library's own included), [1] their bytes, [2] physical chunks created, [3] spare chunks, [4] us in hipMemCreate, [5] us mapping. */
jrx_status jrx_field_alloc(jrx_handle *h, int64_t count, double **out);     /* count doubles */
jrx_status jrx_field_free(jrx_handle *h, double *p);
jrx_status jrx_field_trim(jrx_handle *h);
/* jrx_field_list: the live arrays of the handle (bytes[i] < 0: not chunk-backed), count = how many there are (may exceed cap). */
jrx_status jrx_field_list(jrx_handle *h, int64_t cap, double **ptrs, int64_t *bytes, int64_t *count);
jrx_status jrx_field_stats(jrx_handle *h, int64_t out[6]);

/* Options of the handle: what a caller of solve! may want to choose.  (The A/B switches of the measurements in profiles/ and the test
 * hooks are NOT part of this ABI: include/jrx_tuning.h.)  The library never reads the process environment.  Keys:
 * "kernel_variant" (3D Stokes):
 *   0 = default: fused PT pipeline where it applies (nx >= 48, ny, nz >= 8, and not one of the few nx -- 125 .. 128 -- whose last
 *       62-column tile stays nearly empty while the sweeps' row tiles fill exactly): one kernel runs velocity sweep m + BCs + stress sweep m+1 with ping-pong
 *       state arrays (the handle then owns a second set of the 10 state arrays); with a communicator the exchange
 *       of V follows and the stress nodes next to a received plane are redone; otherwise, and on iterations whose
 *       results are observed, the two z-marching sweeps;
 *   1 = simple one-thread-per-node kernels;  2 = the two sweeps only (z-marching; per-node on blocks up to ~88^3; no ping-pong set);
 *   3 = fused pipeline wherever it is legal (ignores that rule).  All variants produce bit-identical results.
 * "fused_comm" (0/1, default 1): multi-rank runs use the fused pipeline; 0 = split sweeps + hidden communication (same results).
 * "fused_overlap" (0/1/2/3/4, default 3): how the multi-rank fused pipeline places update_halo!(V) (same results in every mode):
 *   3 = neighbour faces inside the kernel, for every rank (4 is accepted as a synonym; viscous-limit form, dt = Inf; other runs use 2): boundary slabs + the exchange on a second stream beside the fused kernel as in 2, but the
 *       kernel's tiles next to a face with a neighbour are launched behind the exchange (the others beside it) and read the received planes themselves: no flow_bcs! launch,
 *       no fix-up launch;
 *   2 = early exchange: the velocity phase alone over the boundary slabs of the faces with a neighbour, flow_bcs! and the whole exchange on a second
 *       stream BESIDE the fused kernel (which recomputes those cells with the same values), then flow_bcs! on the physical faces and the fix-up;
 *   1 = the shell of tiles, BCs and exchange on the second stream while the interior tiles run;  0 = everything behind the kernel, in order.
 * "thermal_fused" (0/1, default 1): jrx_heatdiffusion_PT2d / _PT3d run unobserved iterations as one fused launch with a
 *   library-owned second (T, qT) set; 0 = always compute_flux! and update_T! as two launches (same results).
 * "scratch_sets" (0/1, default 1): 0 forbids every library-owned second state set (3D fused pipeline: + 10 arrays, i.e.
 *   + 10.8 GB at 512^3; 2D fused loop; fused heat diffusion) -- the un-fused kernels then run; same results, less memory.
 * "loop_graphs" (0/1, default 1): runs of unobserved iterations of the launch-bound loops (the 2D loops; the 3D loops on small grids) replay as
 *   captured hipGraphs; same results, shorter gaps between launches.
 * "viscous_limit" (0/1, default 1): with dt = Inf (the reference's purely viscous runs: SolVi3D, Burstedde, TaylorGreen) the 3D visco-elastic
 *   stress kernels (fused iteration, z-marching sweep, boundary layers) do not load the operands that 1/(G dt) = 1/(K dt) = 1/dt = 0 multiply
 *   (old stresses, P0, K, G, Q).  Every driver call first checks those ten arrays in one streaming pass (all of tau_o, P0, Q finite; K, G neither NaN
 *   nor 0): only then do the results equal the general kernels', and only then does this form run -- otherwise the general kernels run and a NaN
 *   there ends the solve with JRX_ERR_NAN exactly as error("NaN(s)") of Stokes3D.jl:162 would.  0 = always the general kernels.
 * "operand_cache" (0/1, default 0): the drivers of the 3D visco-elastic path look at their operand arrays once per call (dt = Inf: may the viscous-limit kernels stand in --
 *   tau_o, P0, Q, eta finite, K, G neither NaN nor 0; any dt: are body-force arrays +0.0 throughout): one streaming pass and a host synchronisation, 3.6 ms at 512^3 -- nothing
 *   inside a solve! of thousands of iterations, 3 % of a 20-iteration batch.  1 = the verdict is kept per (operand pointers, extents, dt) and reused until the caller states that
 *   it has written to one of those arrays: jrx_fields_dirty(h).  The library's own writes (the tau -> tau_o copy at the end of solve!) invalidate it themselves.  Default 0: every call looks.
 * "field_placement" (0/1/2, default 0): backing of the arrays of jrx_field_alloc and of the library's own large arrays: 0 = hipMalloc; 1 = physical chunks
 *   (hipMemCreate) picked at random from a pool and mapped once onto a fresh virtual range per array; 2 = physically contiguous (hipDeviceMallocContiguous; the slowest placement there
 *   is, for A/B runs).  Results never depend on it.
 * "field_chunk_mib" (default 64): size of a physical chunk of "field_placement" = 1 in MiB (0: every array ONE chunk of its own size).  The pool -- chunks for most of the free
 *   memory, created by the first large allocation, dealt at random -- exists for chunks of >= 128 MiB; a caller sets the size of its largest array (for an (nx, ny, nz) block:
 *   (nx + 2)(ny + 2)(nz + 2) x 8 B rounded up to 2 MiB) so that every array is ONE chunk of one common size, which is the arrangement that was measured
 *   (profiles/r05_placement_search.txt section 13, profiles/r06_ten_processes.txt).
 * Read-only counters (jrx_get_option): "stat_fused3d", "stat_fused2d", "stat_thermal_fused", "stat_vep3_fused" = launches of the fused
 *   kernels since jrx_create, "stat_fused3d_visc" = those of "stat_fused3d" that ran the viscous-limit form, "stat_fused3d_inkernel" = those that finished the faces with a neighbour themselves ("fused_overlap" = 3), "stat_visc_checks" /
 *   "stat_visc_fallbacks" = operand checks run / failed (general kernels used), "stat_operand_cache_hits" = driver calls that reused the operand verdict, "stat_graph_replays" = hipGraphLaunch calls,
 *   "stat_sweeps3d" = launches of the 3D z-marching stress and velocity sweeps (k_stress3d_zb, k_velocity3d_zb),
 *   "stat_fused2d_b" = those of "stat_fused2d" that ran the batch form k_fused2d_b (32-bit byte offsets: only below 2^29 nodes, see "fused2d_batch" in jrx_tuning.h),
 *   "stat_fused3d_shfl" / "stat_fused3d_visc_nofold" / "stat_fused3d_visc_nohif" / "stat_fused3d_visc_plain" = those of "stat_fused3d" that ran a form only a tuning switch selects (jrx_tuning.h:
 *   "fused_ylds" = 0; "visc_fold" = 0; "fused_hiface" = 0; both, or a high-face box of "fused_split"), "stat_fused3d_kz12" = those in 12-plane chunks of the 64 x 8 tile ("fused_kz"),
 *   "stat_fused3d_first_none" / "stat_fused3d_first_all" = those of "stat_fused3d_inkernel" that launched no tile / every interior z chunk beside the exchange ("fused_first_pct" = 0 / 100),
 *   "stat_fused3d_split" = fused iterations forked by "fused_split" (four launches each), "stat_hidden3d_bwidth" = split velocity sweeps whose slab widths came from "b_width_x/y/z",
 *   "stat_vep3_edges_kz16" / "_kz8" / "_kz4" = launches of the z-marching 3D VEP edge kernels by chunk depth ("vep3_cfg", or the depth the grid picks), "stat_vep3_edges_mb3" = those of form 1 built
 *   for three blocks per CU, "stat_vep3_edges_peel" = peel launches behind them ("vep3_peel"), "stat_vep3_edges_node" = edge passes run by the one-node-per-thread kernel, of which
 *   "stat_vep3_edges_node_nomap" / "_noxcd" with the plain thread map ("vep3_map" = 0) / without XCD slabs ("vep3_xcd" = 0),
 *   "stat_vep_store_all" = iterations of the VEP and variational loops enqueued with the stores of their output-only arrays only because "vep_store_all" is set,
 *   "stat_weno_calls" / "stat_weno_fused" = jrx_weno5_advection2d calls / those that ran the fused three-launch form,
 *   "stat_weno3d_calls" / "stat_weno3d_fused" = the same for jrx_weno5_advection3d (the 2D pair counts 2D calls only),
 *   "stat_phase_ratios_calls" / "stat_phase_ratios_fused" = jrx_update_phase_ratios2d / 3d calls that launched / those that ran the one-launch form,
 *   "stat_rotate_stress_calls" = jrx_rotate_stress2d / 3d calls that launched,
 *   "stat_rock_fraction_calls" / "stat_topography_advect_calls" / "stat_topography_phase_calls" = jrx_compute_rock_fraction2d / jrx_advect_topography2d /
 *   jrx_update_phases_topography2d calls that launched (their 3D forms jrx_compute_rock_fraction3d / jrx_advect_topography3d / jrx_update_phases_topography3d count in the same three),
 *   "stat_principal_calls" = jrx_principal_stresses2d / 3d calls that launched, "stat_dyrel_launches" = kernels launched by the jrx_dyrel2d_* and jrx_dyrel3d_* entry points,
 *   "stat_stepops_launches" = kernels launched by jrx_pureshear_bc2d / 3d, jrx_free_surface_bcs2d / 3d, jrx_subgrid_characteristic_time and jrx_compute_melt_fraction,
 *   "stat_particles_launches" = kernels launched by the jrx_particles2d_* and jrx_particles3d_* entry points (one each, except the chains of "particles_stress_fused" = 0 and the two subgrid-diffusion calls: 2 / 3, chains 7) -- so that a caller
 *   (and the tests, and bench.py for the kernel it prices) can prove which path ran. */
jrx_status jrx_set_option(jrx_handle *h, const char *key, int64_t value);
/* the caller has written to an operand array (tau_o, P0, Q, K, G, eta, rho g) since the last driver call: a cached verdict of the operand pass ("operand_cache") is dropped */
jrx_status jrx_fields_dirty(jrx_handle *h);
jrx_status jrx_get_option(jrx_handle *h, const char *key, int64_t *value);

/* ------------------------------------------------------------------ block decomposition (host logic; no GPU needed)
 * ImplicitGlobalGrid semantics used by the reference: local arrays of n cells overlap
 * the neighbour by 2 cells; an array of extent nA along a split dimension has overlap
 * ol_A = 2 + (nA - n); update_halo! sends plane ol_A (1-based) to the left neighbour and plane
 * nA - ol_A + 1 to the right one, and receives into planes 1 and nA. */
typedef struct jrx_cart {
    int32_t rank, nprocs;
    int32_t dims[3], coords[3];
    int32_t periods[3];
    int32_t neighbor[3][2];     /* [dim][0=left,1=right], -1 = physical boundary; == rank for a periodic dim with dims[d]==1 */
} jrx_cart;
/* dims = all zeros -> balanced factorisation over the dimensions with n[d] > 1 */
jrx_status jrx_cart_create(int32_t rank, int32_t nprocs, const int64_t n[3], const int32_t dims_in[3],
                           const int32_t periods[3], jrx_cart *out);
/* 0-based plane indices for an array of extent nA in a dimension of n local cells */
jrx_status jrx_halo_planes(int64_t n, int64_t nA, int64_t *send_left, int64_t *send_right,
                           int64_t *recv_left, int64_t *recv_right);
int64_t jrx_n_global(int64_t n, int32_t dims, int32_t periodic);   /* nx_g() */

/* RCCL communicator for the halo exchange + norm all-reduce (one rank per GPU).
 * Rank 0 calls jrx_comm_unique_id and ships the 128 bytes to the others out of band
 * (MPI.Bcast in Julia, torch.distributed in the Python host), then every rank calls init. */
#define JRX_UNIQUE_ID_BYTES 128
jrx_status jrx_comm_unique_id(uint8_t id[JRX_UNIQUE_ID_BYTES]);
jrx_status jrx_comm_init(jrx_handle *h, const uint8_t id[JRX_UNIQUE_ID_BYTES], const jrx_cart *cart);
jrx_status jrx_comm_destroy(jrx_handle *h);
/* The same communicator between PROCESSES of one node with copy engines as transport ("ipc"; one process per rank as the reference runs --
 * mpiexec -n N, test/runtests.jl:73-90 -- and as the Julia extension's MPI ranks would).  Every rank exports one receive buffer per (dimension, side)
 * (hipIpcGetMemHandle), the neighbour maps it and pushes its packed planes into it with hipMemcpyAsync on the exchange's stream; sequence flags in a
 * POSIX shared-memory segment named by `id` order the copies against the unpack kernels (device-side waits with a time-out: a neighbour that never
 * arrives is JRX_ERR_RCCL, not a hang); norms are all-reduced through the segment in rank order.  Rank 0 calls jrx_comm_ipc_id and ships the 128
 * bytes out of band exactly like the RCCL id; every rank then calls jrx_comm_init_ipc.  Needs HSA_ENABLE_IPC_MODE_LEGACY=0 where the driver only
 * supports dmabuf IPC.  Replaces the same call sites as jrx_comm_init. */
jrx_status jrx_comm_ipc_id(uint8_t id[JRX_UNIQUE_ID_BYTES]);
jrx_status jrx_comm_init_ipc(jrx_handle *h, const uint8_t id[JRX_UNIQUE_ID_BYTES], const jrx_cart *cart);
/* The same communicator for ranks that are handles of ONE process (in-process transport): handles[r] becomes rank r of carts[r]
 * (carts[r].rank == r, carts[r].nprocs == n); the handles may sit on one device or on peer-accessible devices.  update_halo! then
 * pushes the packed planes into the neighbour's receive buffer with hipMemcpyAsync / hipMemcpyPeerAsync on the exchange's stream
 * (copy engines instead of send/recv kernels), ordered by events; norms are all-reduced on the host in rank order.  Afterwards every
 * rank must be driven by its own host thread: the entry points that exchange (the solves, jrx_update_halo, jrx_compute_dt) meet on
 * the host and return JRX_ERR_RCCL after 120 s if a neighbour never arrives.  Replaces the same call sites as jrx_comm_init
 * (update_halo! / norm_mpi of src/stokes/Stokes3D.jl:57,120,127-147); jrx_comm_destroy leaves the group. */
jrx_status jrx_comm_init_local(jrx_handle *const *handles, int32_t n, const jrx_cart *carts);
/* the number of ranks of the handle's communicator: ncclCommCount as RCCL itself reports it, or the size of the in-process group
 * (0 = neither) */
jrx_status jrx_comm_count(jrx_handle *h, int32_t *count);
/* update_halo!(A...) for up to 8 arrays, each of extents ext[a][0..2] on a local grid of n cells
 * (call sites: src/stokes/Stokes3D.jl:57,120; src/stokes/Stokes2D.jl:209,268;
 * src/thermal_diffusion/DiffusionPT_solver.jl:110).  Dimension by dimension (x, y, z). */
jrx_status jrx_update_halo(jrx_handle *h, int32_t narrays, double *const *arrays, const int64_t (*ext)[3],
                           const int64_t n[3]);

/* ------------------------------------------------------------------ 3D Stokes, isoviscous visco-elastic variant */
typedef struct jrx_stokes3d_fields {
    double *P, *P0, *divV, *Q;                       /* ni                         (stokes.P, P0, ∇V, Q) */
    double *Vx, *Vy, *Vz;                            /* staggered                  (stokes.V)            */
    double *Ux, *Uy, *Uz;                            /* as V                       (stokes.U)            */
    double *txx, *tyy, *tzz, *tyz, *txz, *txy;       /* @stress(stokes)  -- Voigt order of src/Utils.jl:230-239 */
    double *toxx, *toyy, *tozz, *toyz, *toxz, *toxy; /* @tensor(stokes.τ_o)                              */
    double *exx, *eyy, *ezz, *eyz, *exz, *exy;       /* @strain(stokes)                                  */
    double *eta;                                     /* stokes.viscosity.η, ni                           */
    double *K, *G;                                   /* bulk / shear modulus arrays, ni (may hold Inf)   */
    double *fx, *fy, *fz;                            /* ρg, ni                                           */
    double *RP, *Rx, *Ry, *Rz;                       /* stokes.R                                         */
    double *tyz_c, *txz_c, *txy_c, *toyz_c, *toxz_c, *toxy_c;  /* centre shear copies for multi_copy!, may be NULL */
} jrx_stokes3d_fields;

typedef struct jrx_stokes3d_params {
    int64_t nx, ny, nz;            /* size(stokes.P) on this rank */
    int64_t nxg, nyg, nzg;         /* nx_g(), ny_g(), nz_g() */
    double _dx, _dy, _dz;          /* grid._di.center */
    double dt;                     /* may be Inf */
    double r, theta_dtau, eta_dtau;/* PTStokesCoeffs: r, θ_dτ, ηdτ (src/types/stokes.jl:203-229) */
    double eps_rel, eps_abs;       /* ϵ_rel, ϵ_abs */
    int64_t iterMax, nout;         /* kwargs of solve! (Stokes3D.jl:35-41) */
    uint32_t free_slip, no_slip, periodic;   /* JRX_FACE_* masks of flow_bcs */
    int32_t b_width[3];            /* boundary-slab width for comm/compute overlap (default 4,4,4) */
    int32_t verbose;               /* print the reference's per-check line on rank 0 */
    int32_t displacement_bcs;      /* flow_bcs is a DisplacementBoundaryConditions: displacement2velocity! first (Stokes3D.jl:72), flow_bcs! on U */
} jrx_stokes3d_params;

typedef struct jrx_solve_result {
    int64_t iter;                  /* iterations executed */
    int64_t nchecks;               /* entries filled in the histories below */
    int64_t cap;                   /* capacity of each history buffer (>= iterMax/nout + 1) */
    double *err_evo1; int64_t *err_evo2;
    double *norm_Rx, *norm_Ry, *norm_Rz, *norm_divV;   /* norm_Rz unused in 2D */
    double time_s, av_time_s;      /* wtime0 and wtime0/(iter-1) as in Stokes3D.jl:170,183-184 */
} jrx_solve_result;

/* solve!(stokes, pt_stokes, grid, flow_bcs, ρg, K, G, dt, igg; kwargs) -- src/stokes/Stokes3D.jl:25-186.
 * Runs the whole PT loop on the device: compute_maxloc!(ητ, η) (+halo), then per iteration
 * compute_∇V!, compute_P!, compute_strain_rate!, compute_τ!, compute_V!, velocity2displacement!,
 * flow_bcs!, update_halo!(V), L2 residual norms every nout iterations, and the final τ -> τ_o copy.
 * All outputs the reference leaves in StokesArrays after the call (∇V, ε, R, U included) are
 * left identical. */
jrx_status jrx_stokes3d_solve(jrx_handle *h, const jrx_stokes3d_fields *f, const jrx_stokes3d_params *p,
                              jrx_solve_result *res);

/* Finer-grained entry points (each mirrors reference kernels; used by the parity tests, and by
 * callers that drive the loop themselves).  `etatau` is the ητ array of compute_maxloc!.
 * flags for the fused sweeps: */
enum {
    JRX_OUT_STATE_ONLY = 0,     /* write only the state the next sweep needs (P, τ / V) */
    JRX_OUT_DIAG = 1            /* also write ∇V, ε, RP (stress sweep) / R, U (velocity sweep) */
};
/* compute_∇V! + compute_P! + compute_strain_rate! + compute_τ!  (VelocityKernels.jl:3-6,59-104;
 * PressureKernels.jl:10-15,186-195; StressKernels.jl:149-230) fused into one sweep over ni.+1 */
jrx_status jrx_stokes3d_sweep_stress(jrx_handle *h, const jrx_stokes3d_fields *f, const jrx_stokes3d_params *p,
                                     int32_t flags);
/* compute_V! (VelocityKernels.jl:182-242) + velocity2displacement! (types/displacement.jl:17-28) */
jrx_status jrx_stokes3d_sweep_velocity(jrx_handle *h, const jrx_stokes3d_fields *f, const double *etatau,
                                       const jrx_stokes3d_params *p, int32_t flags);
/* flow_bcs! -- BoundaryConditions.jl:86-100 (no_slip, free_slip, periodic, in that order) */
jrx_status jrx_flow_bcs3d(jrx_handle *h, double *Vx, double *Vy, double *Vz, int64_t nx, int64_t ny, int64_t nz,
                          uint32_t free_slip, uint32_t no_slip, uint32_t periodic);
/* Σx² of Rx,Ry,Rz[2:end-1,2:end-1,2:end-1] and of RP (local part of norm_mpi, Stokes3D.jl:127-142) */
jrx_status jrx_stokes3d_residual_sumsq(jrx_handle *h, const jrx_stokes3d_fields *f, const jrx_stokes3d_params *p,
                                       double out[4]);
/* compute_maxloc!(B, A; window=(1,1,1)) -- src/Utils.jl:409-461 ; nz = 1 selects the 2D form */
jrx_status jrx_compute_maxloc(jrx_handle *h, double *B, const double *A, int64_t nx, int64_t ny, int64_t nz);

/* ------------------------------------------------------------------ 2D Stokes, visco-elastic variant */
typedef struct jrx_stokes2d_fields {
    double *P, *P0, *divV, *Q;
    double *Vx, *Vy, *Ux, *Uy;
    double *txx, *tyy, *txy, *toxx, *toyy, *toxy;
    double *exx, *eyy, *exy;
    double *eta, *K, *G;
    double *fx, *fy;
    double *RP, *Rx, *Ry;
    double *txy_c, *toxy_c;        /* may be NULL */
} jrx_stokes2d_fields;

typedef struct jrx_stokes2d_params {
    int64_t nx, ny, nxg, nyg;
    double _dx, _dy;
    double dt, r, theta_dtau, eta_dtau, eps_rel, eps_abs;
    int64_t iterMax, nout;
    uint32_t free_slip, no_slip, periodic;
    int32_t verbose;
    int32_t displacement_bcs;      /* as in jrx_stokes3d_params (Stokes2D.jl:223) */
    /* Non-uniform Geometry (Geometry(xvi...), src/grid/Cartesian.jl:77-100): device arrays of INVERSE spacings, all six NULL on a uniform grid (then _dx, _dy
     * apply).  [0] _di.vertex[1] (nx), [1] _di.vertex[2] (ny), [2] _di.center[1] (nx-1), [3] _di.center[2] (ny-1), [4] _di.velocity[1][2] (y spacing of
     * the Vx grid, ny+1), [5] _di.velocity[2][1] (x spacing of the Vy grid, nx+1).  Each stencil takes the array the reference's kernel takes
     * (VelocityKernels.jl:3-44,108-180,246-307).  2D drivers only; the one-launch iteration (k_fused2d) is not used on such a grid. */
    const double *inv_spacing[6];
} jrx_stokes2d_params;

/* solve!(stokes, pt_stokes, grid, flow_bcs, ρg, G, K, dt, igg; kwargs) -- src/stokes/Stokes2D.jl:181-325 */
jrx_status jrx_stokes2d_solve(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p,
                              jrx_solve_result *res);
jrx_status jrx_stokes2d_sweep_stress(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau,
                                     const jrx_stokes2d_params *p, int32_t flags);
jrx_status jrx_stokes2d_sweep_velocity(jrx_handle *h, const jrx_stokes2d_fields *f, const double *etatau,
                                       const jrx_stokes2d_params *p, int32_t flags);
/* compute_Res! -- VelocityKernels.jl:246-269 */
jrx_status jrx_stokes2d_compute_res(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p);
jrx_status jrx_flow_bcs2d(jrx_handle *h, double *Vx, double *Vy, int64_t nx, int64_t ny,
                          uint32_t free_slip, uint32_t no_slip, uint32_t periodic);
jrx_status jrx_stokes2d_residual_sumsq(jrx_handle *h, const jrx_stokes2d_fields *f, const jrx_stokes2d_params *p,
                                       double out[3]);

/* ------------------------------------------------------------------ 2D multiphase visco-elasto-plastic Stokes (config 5)
 * solve!(stokes, pt_stokes, grid, flow_bcs, ρg, phase_ratios, rheology, args, dt, igg; kwargs)
 * -- src/stokes/Stokes2D.jl:577-866 with update_stresses_center_vertex_ps! (src/stokes/StressKernels.jl:992-1144),
 * compute_P! phase-ratio form (PressureKernels.jl:47-106), update_viscosity_τII! (rheology/Viscosity.jl:67-106,382-418)
 * and the post-loop epilogue (vorticity, shear2center!, accumulate_tensor!, accumulate_vol!, multi_copy!).
 * The rheology is passed as a table instead of GeoParams objects: per phase a LinearViscous viscosity, ConstantElasticity
 * (G, Kb) and an optional DruckerPrager_regularised(C, ϕ, ψ, η_vp) -- what test/test_shearband2D.jl uses.  Phase ratios
 * are JustPIC's CellArray layout: phase index fastest, [nphase][nx][ny] at centres and [nphase][nx+1][ny+1] at vertices. */
#define JRX_MAXPHASE 8
typedef struct jrx_rheology {
    int32_t nphase;
    double eta[JRX_MAXPHASE], G[JRX_MAXPHASE], Kb[JRX_MAXPHASE];
    int32_t is_pl[JRX_MAXPHASE];
    double C[JRX_MAXPHASE], sinphi[JRX_MAXPHASE], cosphi[JRX_MAXPHASE], sinpsi[JRX_MAXPHASE], eta_vp[JRX_MAXPHASE];
    /* ---- appended in round 2; a zero-initialised tail gives the round-1 behaviour (LinearViscous, NoSoftening, ρg owned by the caller) ----
     * Density and gravity -- compute_ρg! / update_ρg! (rheology/BuoyancyForces.jl:37-60,153-167).  has_density = 0: the ρg arrays
     * are the caller's and never recomputed.  rho_kind: 0 ConstantDensity(rho0), 1 PT_Density rho0 (1 - alpha (T - T0) + beta (P - P0)),
     * 2 T_Density rho0 (1 - alpha (T - T0)), 3 Compressible_Density rho0 exp(beta (P - P0)) [GeoParams forms, assumed].
     * gravity = compute_gravity(first(rheology)): a scalar, it fills the last component of ρg (BuoyancyForces.jl:69-70). */
    int32_t has_density;
    int32_t rho_kind[JRX_MAXPHASE];
    double rho0[JRX_MAXPHASE], alpha[JRX_MAXPHASE], beta[JRX_MAXPHASE], T0[JRX_MAXPHASE], P0[JRX_MAXPHASE];
    double gravity;
    /* Strain softening of the cohesion and of the friction angle, evaluated at the accumulated plastic strain EII_pl (the EII keyword
     * of compute_yieldfunction_phase, StressKernels.jl:1053-1105; GeoParams softening_C / softening_ϕ, forms assumed):
     * kind 0 NoSoftening, 1 LinearSoftening((a = min, b = max), (c = lo, d = hi)): b for EII <= lo, a for EII >= hi, linear between;
     * 2 NonLinearSoftening(a = ξ₀, b = Δ, c = μ, d = σ) = ξ₀ - Δ/2 erfc(-(EII - μ)/σ).  phi_deg is the unsoftened friction angle. */
    int32_t softC_kind[JRX_MAXPHASE], softphi_kind[JRX_MAXPHASE];
    double softC_a[JRX_MAXPHASE], softC_b[JRX_MAXPHASE], softC_c[JRX_MAXPHASE], softC_d[JRX_MAXPHASE];
    double softphi_a[JRX_MAXPHASE], softphi_b[JRX_MAXPHASE], softphi_c[JRX_MAXPHASE], softphi_d[JRX_MAXPHASE], phi_deg[JRX_MAXPHASE];
    /* Creep law of the viscous element for compute_viscosity! / compute_viscosity_τII! with dt = Inf (rheology/Viscosity.jl:142-167):
     * visc_kind 0 LinearViscous(eta); 1 Arrhenius: eta exp((Ea + P Va)/(Rgas T) - Ea/(Rgas Tref)), clamped to [visc_lo, visc_hi]
     * (the CustomRheology of test/test_WENO5.jl:37-42 with depth = 0);
     * 2 power-law creep (GeoParams DislocationCreep with r = 0; DiffusionCreep is n = 1 with the grain-size factor folded into A):
     *   compute_εII: ε = creep_A (τII creep_FT)^creep_n exp(-(Ea + P Va)/(Rgas T)) / creep_FE
     *   compute_τII: τ = creep_A^(-1/n) (εII creep_FE)^(1/n) exp((Ea + P Va)/(n Rgas T)) / creep_FT
     *   compute_viscosity_τII = τII / (2 ε(τII)),  compute_viscosity_εII = τ(εII) / (2 εII)      [forms ASSUMED, parity unpinned]
     * (the 2D single-material driver hands its in-loop compute_viscosity_τII! the strain-rate invariant, as the reference's _compute_viscosity! does.)
     * FT, FE: GeoParams' apparatus corrections (AxialCompression √3, 2/√3; SimpleShear 2, 2; Invariant 1, 1).  One creep element per phase.
     * The invariant a law of kind 2 is evaluated at is the one the reference's kernels form (Viscosity.jl:382-418,455-503): compute_viscosity! from the strain
     * rate, update_viscosity_τII! from the stress, eps() on the normal components of an all-zero tensor. */
    int32_t visc_kind[JRX_MAXPHASE];
    double Ea[JRX_MAXPHASE], Va[JRX_MAXPHASE], Tref[JRX_MAXPHASE], Rgas[JRX_MAXPHASE], visc_lo[JRX_MAXPHASE], visc_hi[JRX_MAXPHASE];
    double creep_A[JRX_MAXPHASE], creep_n[JRX_MAXPHASE], creep_FT[JRX_MAXPHASE], creep_FE[JRX_MAXPHASE];      /* visc_kind 2 */
} jrx_rheology;

typedef struct jrx_vep2d_fields {
    double *P, *P0, *divV, *Q;                     /* stokes.P, P0, ∇V, Q */
    double *Vx, *Vy, *Ux, *Uy;
    double *exx, *eyy, *exy, *exy_c;               /* stokes.ε: xx, yy (centres), xy (vertices), xy_c */
    double *eplxx, *eplyy, *eplxy, *eplxy_c;       /* stokes.ε_pl */
    double *dexy_c, *dexy;                         /* stokes.Δε.xy_c, .xy (shear2center! only; may be NULL) */
    double *txx, *tyy, *txy, *txy_c, *tII;         /* stokes.τ: xx, yy, xy (vertices), xy_c, II */
    double *toxx, *toyy, *toxy, *toxy_c;           /* stokes.τ_o */
    double *eta, *eta_v, *eta_vep;                 /* stokes.viscosity.η, ηv (may be NULL), η_vep */
    double *EII_pl, *evol_pl, *EVol_pl;            /* stokes.EII_pl, ε_vol_pl, EVol_pl */
    double *fx, *fy;                               /* ρg */
    double *RP, *Rx, *Ry;
    double *omega_xy;                              /* stokes.ω.xy (may be NULL) */
    double *phase_c, *phase_v;                     /* phase_ratios.center / .vertex */
    const double *T;                               /* args.T at the cell centres (ni) for the density laws; may be NULL (T = 0) */
    double *dexx, *deyy, *divU;                    /* strain_increment variant: Δε.xx, Δε.yy, stokes.∇U (ni); may be NULL otherwise */
    /* ---- appended with the thermal stresses; a zero-initialised tail gives the isothermal pressure equation ----
     * args.ΔT: compute_P! of the multiphase driver gains the thermal-expansion source α ΔT / dt (PressureKernels.jl:64-85,129-152,197-206; handed over
     * by Stokes2D.jl:663-676): rhs = (-∇V + (α_c * (ΔT * _dt))) + (Q * _dt), with α_c = fn_ratio(get_thermal_expansion, rheology, phase_ratio[I]) -- the phase-ratio
     * sum with the early-return and skip rules of the density average; α of a phase is its `alpha` for the density kinds PT_Density and T_Density and 0 for
     * ConstantDensity and Compressible_Density [GeoParams form, assumed]; rho_kind and alpha are read whether or not has_density is set (ρg may stay the caller's).  For ratios that
     * sum to one this is the plain phase-ratio sum of PressureKernels.jl:147.  ΔT is read at the cell's own [i, j] (PressureKernels.jl:149): cell-centred (ni), or
     * thermal.ΔT itself (ni .+ 2) with p->dT_ghosted = 1, then still unshifted.  NULL: the instantiations and the bits of the isothermal driver.
     * Read by jrx_stokes2d_vep_solve (all its forms) and jrx_vep2d_compute_P only: the single-phase driver hands compute_P! no args (Stokes2D.jl:420), the ΔT
     * methods of the variational drivers are commented out in the reference, and the DYREL drivers refuse ΔT by the members of their own struct. */
    const double *dT;
    /* args.melt_fraction: a no-op without ΔT, as in the reference (PressureKernels.jl:108-127).  Together with ΔT the reference takes α(ϕ) from GeoParams in a
     * form nothing under it states: refused with JRX_ERR_ARG before anything is launched. */
    const double *melt_fraction;
} jrx_vep2d_fields;

typedef struct jrx_vep2d_params {
    int64_t nx, ny, nxg, nyg;
    double _dx, _dy;
    double dt, r, theta_dtau, eta_dtau, eps_rel, eps_abs;
    int64_t iterMax, iterMin, nout;                /* kwargs (Stokes2D.jl:588-599): iterMax=50e3, iterMin=100, nout=500 */
    uint32_t free_slip, no_slip, periodic;
    double lambda_relaxation, viscosity_relaxation, cutoff_lo, cutoff_hi;
    int32_t verbose;
    int32_t free_surface;                          /* kwarg free_surface: compute_V! / compute_Res! get dt * free_surface (Stokes2D.jl:773,797) */
    int32_t displacement_bcs;                      /* flow_bcs is a DisplacementBoundaryConditions: V = U / dt first, flow_bcs! acts on U */
    int32_t T_ghosted;                             /* args.T is thermal.T (nx+2, ny+2), indexed as the reference does (densities at the cell's own [i, j]) */
    int32_t strain_increment;                      /* kwarg strain_increment (jrx_stokes2d_vep_solve only; Stokes2D.jl:588,659-734, StressKernels.jl:1147-1302): strains
                                                    * from the displacement increments U = V dt, Δε form of the stress update; U and its BCs are refreshed every iteration */
    const double *inv_spacing[6];                  /* non-uniform Geometry: as in jrx_stokes2d_params (all NULL: uniform); not with strain_increment */
    int32_t dT_ghosted;                            /* f->dT = args.ΔT is thermal.ΔT (nx+2, ny+2), read at the cell's own [i, j]; 0: cell-centred (ni) */
} jrx_vep2d_params;

jrx_status jrx_stokes2d_vep_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p,
                                  jrx_solve_result *res);
/* solve!(stokes, pt_stokes, grid, flow_bcs, ρg, rheology::MaterialParams, args, dt, igg; kwargs) -- src/stokes/Stokes2D.jl:345-557: the 2D
 * single-phase visco-elasto-plastic driver built on compute_τ_nonlinear! and center2vertex! (test/test_WENO5.jl:226-291).  The rheology is
 * phase 0 of the table (creep law, ConstantElasticity, optional DruckerPrager_regularised, density); phase_c / phase_v are not read.
 * f->T = args.T: cell-centred (ni), or thermal.T (ni.+2) with p->T_ghosted = 1 -- then read at [i, j] by the density and at [i+1, j+1]
 * by the viscosity, as the reference's two argument helpers do.  f->dT and f->melt_fraction are not read: this driver hands compute_P! no args
 * (Stokes2D.jl:420). */
jrx_status jrx_stokes2d_nonlinear_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p,
                                        jrx_solve_result *res);
/* update_stresses_center_vertex_ps! alone (θ, λ, λv are caller arrays of extents ni, ni, ni.+1) -- for parity tests */
jrx_status jrx_vep2d_update_stresses(jrx_handle *h, const jrx_vep2d_fields *f, const double *theta, double *lambda, double *lambda_v,
                                     const jrx_rheology *rh, const jrx_vep2d_params *p);
/* the phase averages (K, G, and with f->dT the thermal source α_c * (ΔT * _dt)) and one evaluation of compute_∇V! + compute_P! (phase form, thermal form with
 * f->dT: PressureKernels.jl:87-106,129-152) + compute_strain_rate! on the caller's arrays -- for parity tests.  θ (ni) is the pressure compute_P! updates in
 * place; ητ is taken as the driver's first iteration takes it (compute_maxloc! of f->eta).  Writes θ, ∇V, RP, ε.xx, ε.yy, ε.xy and nothing else;
 * reads f->Q, f->P0, V, η, the centre phase ratios.  f->dT with f->melt_fraction is refused as in the solve. */
jrx_status jrx_vep2d_compute_P(jrx_handle *h, const jrx_vep2d_fields *f, double *theta, const jrx_rheology *rh, const jrx_vep2d_params *p);
/* compute_τ_nonlinear! 2D alone: single phase (multiphase = 0; StressKernels.jl:266-307, uses rheology phase 0) or phases at
 * the cell centres (multiphase = 1; :310-351) with _compute_τ_nonlinear! (rheology/StressUpdate.jl:2-57).  Centre-only
 * visco-elasto-plastic update: writes τ.xx, τ.yy, τ.xy_c, τ.II, η_vep, ε_pl.xx, ε_pl.yy, ε_pl.xy[i,j], λ and θ (caller
 * arrays of extent ni).  τ_o.xy and ε_pl.xy are the vertex arrays addressed with the centre index, as the reference's
 * caller passes them (Stokes2D.jl:442-458).  Softening laws are not modelled (NoSoftening). */
jrx_status jrx_compute_tau_nonlinear2d(jrx_handle *h, const jrx_vep2d_fields *f, double *theta, double *lambda, const jrx_rheology *rh,
                                       const jrx_vep2d_params *p, int32_t multiphase);
/* center2vertex!(vertex, center) 2D (Interpolations.jl:101-114): vertex is (nx+1, ny+1), center (nx, ny) */
jrx_status jrx_center2vertex2d(jrx_handle *h, double *vertex, const double *center, int64_t nx, int64_t ny);
/* tensor_invariant!(A): II = second_invariant_staggered(xx, yy, gather(xy)) -- StressKernels.jl:443-470 */
jrx_status jrx_tensor_invariant2d(jrx_handle *h, double *II, const double *xx, const double *yy, const double *xy, int64_t nx, int64_t ny);
/* compute_viscosity! (fn_viscosity = compute_viscosity_εII) for the table rheology: η <- ν·η_phase + (1-ν)·η, clamped to the cutoff; creep laws that read
 * fields take T (f->T with p->T_ghosted as in the solve), P = f->P and the invariant of @strain_center as the reference's kernel does (Viscosity.jl:382-418) */
jrx_status jrx_vep2d_compute_viscosity(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu);
/* the same with fn_viscosity = compute_viscosity_τII (update_viscosity_τII!, Viscosity.jl:67-106): a power-law creep is evaluated at the invariant of
 * @stress_center (vertices: τ.xy alone, the PT solvers leave τ.xx_v, τ.yy_v zero) instead of the strain rate's; identical for the other creep laws */
jrx_status jrx_vep2d_compute_viscosity_tauII(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu);

/* ------------------------------------------------------------------ 2D variational Stokes (free surface through a rock-ratio mask)
 * solve_VariationalStokes!(stokes, pt_stokes, grid, flow_bcs, ρg, phase_ratios, ϕ::RockRatio, rheology, args, dt, igg; air_phase, kwargs)
 * -- src/variational_stokes/Stokes2D.jl:24-314: the multiphase visco-elasto-plastic driver above with the rock ratio ϕ on ∇V, the strain
 * rates, the stress update and the velocity update (variational_stokes/VelocityKernels.jl:6-59,332-401, StressKernels.jl:2-170,
 * MiniKernels.jl, mask.jl:168-254), residual norms over the valid nodes only, and the air_phase correction of the viscosity
 * (rheology/Viscosity.jl:403-405,638-650).  Built: 2D, one block, uniform spacing, strain-rate form.  Status JRX_ERR_ARG, with a text that
 * names it, for: p->inv_spacing non-NULL, p->strain_increment, a handle with a communicator, a DruckerPragerCap phase (the table has no such law: a caller
 * that meets one marks the phase with is_pl = 2, and any is_pl other than 0 or 1 is refused), and -- beyond the reference, where correct_phase_ratio would index
 * out of range -- an air_phase outside 0..nphase (the solve and jrx_vep2d_compute_viscosity_air; jrx_update_rock_ratio accepts any value, as compute_rock_ratio does).
 * ϕ (variational_stokes/mask.jl:1-42): center (nx, ny), vertex (nx+1, ny+1), Vx (nx+1, ny), Vy (nx, ny+1) -- no ghost nodes. */
typedef struct jrx_rock_ratio2d {
    const double *center, *vertex, *Vx, *Vy;
} jrx_rock_ratio2d;
/* compute_rock_ratio / update_rock_ratio_cv! / _update_rock_ratio! (variational_stokes/mask.jl:112-157) for one member of ϕ, any dimension:
 * dst[t] = 1 - phase[air_phase - 1 + nphase * t] (CellArray layout, phase index fastest; air_phase is 1-based), zeroed when <= 1e-5; 1.0 when
 * air_phase is outside 1..nphase; clamp != 0: clamped to [0, 1] (the velocity and shear members; center and vertex are not clamped). */
jrx_status jrx_update_rock_ratio(jrx_handle *h, double *dst, const double *phase, int32_t nphase, int32_t air_phase, int64_t count, int32_t clamp);
/* _solve_VS! (variational_stokes/Stokes2D.jl:24-314).  air_phase: 1-based index of the air phase, 0 = none.  The norms are taken over
 * Rx[ϕ.Vx[2:end-1, :] .> 0], Ry[ϕ.Vy[:, 2:end-1] .> 0], RP[ϕ.center .> 0] and divided by the unmasked counts (:59-61,255-259). */
jrx_status jrx_stokes2d_vs_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                                 const jrx_vep2d_params *p, int32_t air_phase, jrx_solve_result *res);
/* masked compute_∇V! + compute_strain_rate! alone (variational_stokes/VelocityKernels.jl:6-59): writes ∇V, ε.xx, ε.yy, ε.xy; zero at invalid nodes -- for parity tests */
jrx_status jrx_vs2d_strain_rates(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const jrx_vep2d_params *p);
/* masked update_stresses_center_vertex! 2D alone (variational_stokes/StressKernels.jl:2-170; θ, λ, λv are caller arrays of extents ni, ni, ni.+1).
 * At an invalid centre τ (xx, yy, xy_c), ε_pl (xx, yy, and xy at the centre's own index), Pr_c = f->P, η_vep and ε_vol_pl are zeroed and τ.II is
 * left; at an invalid vertex only τ.xy is zeroed -- for parity tests */
jrx_status jrx_vs2d_update_stresses(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const double *theta, double *lambda,
                                    double *lambda_v, const jrx_rheology *rh, const jrx_vep2d_params *p);
/* masked compute_V! with dt alone (variational_stokes/VelocityKernels.jl:332-401): V, Rx, Ry; etatau is ητ (ni); the free-surface term takes
 * dt * free_surface = p->free_surface ? p->dt : 0 -- for parity tests */
jrx_status jrx_vs2d_compute_V(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rock_ratio2d *phi, const double *etatau, const jrx_vep2d_params *p);
/* compute_viscosity! (tauII = 0) / update_viscosity_τII! (tauII != 0) with the air_phase keyword (rheology/Viscosity.jl:382-418): the ratios of a
 * node go through correct_phase_ratio (:638-650) first -- all zero where the air ratio ≈ 1, else the air entry dropped and the rest
 * renormalised.  air_phase = 0: the arithmetic of jrx_vep2d_compute_viscosity / _tauII. */
jrx_status jrx_vep2d_compute_viscosity_air(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_rheology *rh, const jrx_vep2d_params *p, double nu,
                                           int32_t air_phase, int32_t tauII);

/* ------------------------------------------------------------------ 3D multiphase visco-elasto-plastic Stokes
 * solve!(stokes, pt_stokes, grid, flow_bcs, ρg, phase_ratios, rheology, args, dt, igg; kwargs) for 3D grids --
 * src/stokes/Stokes3D.jl:447-668 with update_stresses_center_vertex_ps! 3D (src/stokes/StressKernels.jl:604-989), as
 * test/test_shearband3D_MPI.jl drives it.  Same rheology table as the 2D driver.  Extents: centres ni; edge arrays
 * yz (nx, ny+1, nz+1), xz (nx+1, ny, nz+1), xy (nx+1, ny+1, nz); phase arrays [nphase][extent] with the phase index
 * fastest (JustPIC CellArray).  Pointers marked optional may be NULL. */
typedef struct jrx_vep3d_fields {
    double *P, *P0, *divV, *Q;
    double *Vx, *Vy, *Vz, *Ux, *Uy, *Uz;
    double *exx, *eyy, *ezz, *eyz, *exz, *exy;            /* ε: normals at centres, shear on edges */
    double *eyz_c, *exz_c, *exy_c;                        /* optional: shear2center!(stokes.ε) targets */
    double *eplxx, *eplyy, *eplzz, *eplyz, *eplxz, *eplxy;/* ε_pl */
    double *eplyz_c, *eplxz_c, *eplxy_c;                  /* optional */
    double *deyz, *dexz, *dexy, *deyz_c, *dexz_c, *dexy_c;/* optional: Δε shear and its centre copies */
    double *txx, *tyy, *tzz, *tyz, *txz, *txy;            /* τ: normals at centres, shear on edges */
    double *tyz_c, *txz_c, *txy_c, *tII;                  /* τ shear at centres, second invariant */
    double *toxx, *toyy, *tozz, *toyz, *toxz, *toxy, *toyz_c, *toxz_c, *toxy_c;
    double *eta, *eta_vep;
    double *EII_pl, *evol_pl, *EVol_pl;
    double *fx, *fy, *fz;                                 /* ρg */
    double *RP, *Rx, *Ry, *Rz;
    double *omega_yz, *omega_xz, *omega_xy;               /* optional: vorticity on the edges */
    const double *phase_c, *phase_yz, *phase_xz, *phase_xy;
    const double *T;                                      /* args.T at the cell centres (ni); may be NULL (T = 0) */
    /* ---- appended with the thermal stresses; a zero-initialised tail gives the isothermal pressure equation ----
     * args.ΔT and args.melt_fraction as in jrx_vep2d_fields (compute_P! of Stokes3D.jl:518-531, PressureKernels.jl:129-152,197-206): ΔT at the cell's own
     * [i, j, k], of extent ni or -- p->dT_ghosted = 1 -- ni .+ 2.  Read by jrx_stokes3d_vep_solve (fused, three-kernel and multi-rank paths) and jrx_vep3d_compute_P. */
    const double *dT;
    const double *melt_fraction;
} jrx_vep3d_fields;

typedef struct jrx_vep3d_params {
    int64_t nx, ny, nz, nxg, nyg, nzg;
    double _dx, _dy, _dz;
    double dt, r, theta_dtau, eta_dtau, eps_rel, eps_abs;
    int64_t iterMax, nout;
    uint32_t free_slip, no_slip, periodic;
    double lambda_relaxation, viscosity_relaxation, cutoff_lo, cutoff_hi;
    int32_t verbose;
    int32_t displacement_bcs;
    int32_t T_ghosted;             /* f->T = args.T is thermal.T (ni .+ 2), as the miniapps pass it (RisingBlob3D/Blob3D.jl:355): update_ρg! reads it at the cell's own
                                    * [i, j, k], unshifted (getindex_NamedTuple(args, I...), BuoyancyForces.jl:52); 0: cell-centred (ni) */
    int32_t b_width[3];            /* kwargs.b_width (Stokes3D.jl:460): boundary-slab widths of the hidden update_halo!(V) (multi-rank runs; <= 0: 4) */
    int32_t dT_ghosted;            /* f->dT = args.ΔT is thermal.ΔT (ni .+ 2), read at the cell's own [i, j, k]; 0: cell-centred (ni) */
} jrx_vep3d_params;

jrx_status jrx_stokes3d_vep_solve(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rheology *rh, const jrx_vep3d_params *p,
                                  jrx_solve_result *res);
/* update_stresses_center_vertex_ps! 3D alone (θ, λ of extent ni; λv = {yz, xz, xy} edge arrays) -- for parity tests.
 * Every update reads the stresses of the previous call (the reference's single launch races on neighbouring values). */
jrx_status jrx_vep3d_update_stresses(jrx_handle *h, const jrx_vep3d_fields *f, const double *theta, double *lambda, double *const lambda_v[3],
                                     const jrx_rheology *rh, const jrx_vep3d_params *p);
/* jrx_vep2d_compute_P one dimension up: writes θ (ni), ∇V, RP and the six components of ε; nothing else */
jrx_status jrx_vep3d_compute_P(jrx_handle *h, const jrx_vep3d_fields *f, double *theta, const jrx_rheology *rh, const jrx_vep3d_params *p);
/* compute_viscosity! 3D (εII form; ..._tauII: update_viscosity_τII!) for the table rheology: η <- ν·η_phase + (1-ν)·η, clamped to the cutoff; creep laws that
 * read fields: T, P at the cell, invariant of @strain / @stress with the edge components gathered (Viscosity.jl:455-503) */
jrx_status jrx_vep3d_compute_viscosity(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rheology *rh, const jrx_vep3d_params *p, double nu);
jrx_status jrx_vep3d_compute_viscosity_tauII(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rheology *rh, const jrx_vep3d_params *p, double nu);
/* tensor_invariant!(A) 3D -- StressKernels.jl:472-487 */
jrx_status jrx_tensor_invariant3d(jrx_handle *h, double *II, const double *xx, const double *yy, const double *zz, const double *yz,
                                  const double *xz, const double *xy, int64_t nx, int64_t ny, int64_t nz);

/* ------------------------------------------------------------------ 3D variational Stokes (the 2D section above, one dimension up; it follows the 3D
 * multiphase structs it takes)
 * solve_VariationalStokes!(stokes, pt_stokes, grid::Geometry{3}, flow_bcs, ρg, phase_ratios, ϕ::RockRatio, rheology, args, dt, igg; air_phase, kwargs)
 * -- src/variational_stokes/Stokes3D.jl:14-238: the 3D multiphase driver with the rock ratio ϕ on ∇V, the strain rates, the stress update and
 * the velocity update (variational_stokes/VelocityKernels.jl:6-12,96-154, StressKernels.jl:173-508, mask.jl:180-186,220-269,324-392) and the
 * air_phase correction of the viscosity (rheology/Viscosity.jl:638-650).  Unlike the 2D driver: no iterMin (`while iter < 2 || (... && iter <= iterMax)`),
 * norms over ALL nodes -- norm_Ri = ‖Ri[2:end-1, 2:end-1, 2:end-1]‖ / sqrt((nx_g-1)(ny_g-1)(nz_g-1)), norm_∇V = ‖RP‖ / length(RP) (:175-181) --, relλ the
 * literal 0.2 (:137; p->lambda_relaxation is not read), no free-surface stabilisation.
 * The momentum kernel is NOT the reference's text: its masked 3D compute_V! (VelocityKernels.jl:408-487) calls _av_x / _av_y / _av_z(A, ϕ, ...) that nothing
 * defines, its masked d_xi / d_yi / d_zi resolve to the N-dimensional forms of MiniKernels.jl:20-27, which in 3D difference across two planes, and they read
 * τxy[..., k+1] at k = nz; no test or miniapp of the reference calls it.  Built instead: the working masked 2D kernel (:355-399) one dimension up, on the
 * index triples of the unmasked 3D kernel (src/stokes/VelocityKernels.jl:215-238) -- at a valid Vx node (isvalid_vx(ϕ, i+1, j, k), (i, j, k) <= size(Rx))
 *   Rx[i,j,k] = ((τxx ϕc)[i+1,j,k] - (τxx ϕc)[i,j,k]) _dx + ((τxy ϕxy)[i+1,j+1,k] - (τxy ϕxy)[i+1,j,k]) _dy + ((τxz ϕxz)[i+1,j,k+1] - (τxz ϕxz)[i+1,j,k]) _dz
 *               - ((P ϕc)[i+1,j,k] - (P ϕc)[i,j,k]) _dx - 0.5 ((fx ϕc)[i,j,k] + (fx ϕc)[i+1,j,k]),     Vx[i+1,j+1,k+1] += Rx[i,j,k] ηdτ / av_x(ητ)   (ητ unmasked)
 * and Rx = Vx = 0 at an invalid one; y and z alike with isvalid_vy(ϕ, i, j+1, k), isvalid_vz(ϕ, i, j, k+1).
 * Built: 3D, one block, uniform spacing.  Status JRX_ERR_ARG, with a text that names it, for: inverse spacings that are not positive finite scalars (how the
 * binding hands over a non-uniform Geometry, for which this struct has no arrays), a handle with a communicator, a DruckerPragerCap phase (is_pl = 2), an
 * air_phase outside 0..nphase, fewer than 3 cells in a dimension.
 * ϕ (variational_stokes/mask.jl:1-42): center ni, vertex ni .+ 1, Vx (nx+1, ny, nz), Vy (nx, ny+1, nz), Vz (nx, ny, nz+1), yz (nx, ny+1, nz+1),
 * xz (nx+1, ny, nz+1), xy (nx+1, ny+1, nz) -- no ghost nodes. */
typedef struct jrx_rock_ratio3d {
    const double *center, *vertex, *Vx, *Vy, *Vz, *yz, *xz, *xy;
} jrx_rock_ratio3d;
/* _solve_VS! (variational_stokes/Stokes3D.jl:14-238).  air_phase: 1-based index of the air phase, 0 = none. */
jrx_status jrx_stokes3d_vs_solve(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                                 const jrx_vep3d_params *p, int32_t air_phase, jrx_solve_result *res);
/* masked compute_∇V! + compute_strain_rate! 3D alone (variational_stokes/VelocityKernels.jl:6-12,96-154): ∇V is zero at an invalid centre; the six
 * strain rates are written at valid nodes only and keep their values elsewhere (the reference's kernel does not zero them) -- for parity tests */
jrx_status jrx_vs3d_strain_rates(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const jrx_vep3d_params *p);
/* masked update_stresses_center_vertex! 3D alone (variational_stokes/StressKernels.jl:173-508; θ, λ of extent ni; λv = {yz, xz, xy} edge arrays), relλ = 0.2.
 * An invalid edge zeroes its τ alone; an invalid centre zeroes Pr_c = f->P, η_vep, ε_vol_pl, the six τ centre arrays and the six entries of
 * @plastic_strain -- the shear ones are the EDGE arrays at the centre's own index -- and leaves τ.II.  Every update reads the stresses of the previous
 * call, as jrx_vep3d_update_stresses -- for parity tests */
jrx_status jrx_vs3d_update_stresses(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const double *theta, double *lambda,
                                    double *const lambda_v[3], const jrx_rheology *rh, const jrx_vep3d_params *p);
/* the masked momentum kernel alone (replaces variational_stokes/VelocityKernels.jl:408-487 in the form stated above): V, Rx, Ry, Rz; etatau is ητ (ni) -- for parity tests */
jrx_status jrx_vs3d_compute_V(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rock_ratio3d *phi, const double *etatau, const jrx_vep3d_params *p);
/* compute_viscosity! (tauII = 0) / update_viscosity_τII! (tauII != 0) 3D with the air_phase keyword (rheology/Viscosity.jl:455-503): the ratios of a cell go
 * through correct_phase_ratio (:638-650) first.  air_phase = 0: the arithmetic of jrx_vep3d_compute_viscosity / _tauII, bit for bit. */
jrx_status jrx_vep3d_compute_viscosity_air(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_rheology *rh, const jrx_vep3d_params *p, double nu,
                                           int32_t air_phase, int32_t tauII);

/* ------------------------------------------------------------------ 2D PT heat diffusion */
typedef struct jrx_thermal2d_fields {
    double *T, *Told, *dT;                 /* (nx+2, ny+2): thermal.T, Told, ΔT */
    double *qTx, *qTx2;                    /* (nx+1, ny)   */
    double *qTy, *qTy2;                    /* (nx, ny+1)   */
    double *H, *shear_heating, *ResT;      /* (nx, ny)     */
    double *K, *rhoCp;                     /* (nx, ny); unused (may be NULL) in the rheology form */
    double *thetar_dtau, *dtau_rho;        /* (nx, ny): pt_thermal.θr_dτ, dτ_ρ */
    /* optional (NULL = absent; the one-launch iterations are not used when any is given) */
    const double *adiabatic;               /* (nx, ny): thermal.adiabatic, the term + adiabatic * T of the rheology forms (DiffusionPT_kernels.jl:553-601,631-668) */
    const double *dirichlet_mask;          /* (nx+2, ny+2): thermal_bc.dirichlet.mask -- cells with mask != 0 take T = (1 - m) T + m value instead of the update
                                            * and have ResT = 0 (Dirichlet.jl:72-105, mask/mask.jl:47-50) */
    const double *dirichlet_value;         /* (nx+2, ny+2) values; NULL with a ConstantDirichletBoundaryCondition (params.dirichlet_const) */
} jrx_thermal2d_fields;

typedef struct jrx_thermal2d_params {
    int64_t nx, ny;
    double _dx, _dy;
    double dt, eps;                        /* pt_thermal.ϵ */
    int64_t iterMax, nout;
    /* faces in the order left, right, top, bot (2D: bot <-> j = 1) */
    int32_t no_flux[4];
    int32_t constant_value_on[4]; double constant_value[4];
    int32_t constant_flux_on[4];  double constant_flux[4];
    int32_t periodic[4];
    /* 0: array-coefficient form (DiffusionPT_solver.jl:34-149);
     * 1: rheology form restricted to constant k, constant Cp, rho = rho0*(1 - alpha*(T - T0))
     *    (DiffusionPT_solver.jl:181-305 as evaluated by test/test_diffusion2D.jl) */
    int32_t rheology_form;
    double k_const, Cp, rho0, alpha, T0;
    int32_t verbose;
    double dirichlet_const;                /* value of a ConstantDirichletBoundaryCondition (read where dirichlet_mask != 0 and dirichlet_value is NULL) */
    /* Non-uniform Geometry (device arrays of inverse spacings, all four NULL on a uniform grid): [0], [1] = _di.center x (nx-1), y (ny-1): compute_flux! reads them
     * at clamp(i, 1, nx-1) (DiffusionPT_kernels.jl:338,354,405,433,482,510); [2], [3] = _di.vertex x (nx), y (ny): update_T! of the rheology / phase forms and
     * check_res! (:579-580,616,647-648).  Not with the array form (K, ρCp arrays): its update_T! indexes _di.center beyond its extent in the reference (:532). */
    const double *inv_spacing[4];
} jrx_thermal2d_params;

/* heatdiffusion_PT!(thermal, pt_thermal, thermal_bc, K, ρCp | rheology, args, dt, grid; kwargs) */
jrx_status jrx_heatdiffusion_PT2d(jrx_handle *h, const jrx_thermal2d_fields *t, const jrx_thermal2d_params *p,
                                  int64_t *iter_count, double *norm_ResT, int64_t cap, int64_t *nnorms);
/* thermal_bcs! -- BoundaryConditions.jl:39-53 */
jrx_status jrx_thermal_bcs2d(jrx_handle *h, double *T, const jrx_thermal2d_params *p);
/* one PT iteration: compute_flux! + update_T! + thermal_bcs! (DiffusionPT_solver.jl:236-261) */
jrx_status jrx_thermal2d_iteration(jrx_handle *h, const jrx_thermal2d_fields *t, const jrx_thermal2d_params *p);
/* check_res! (DiffusionPT_kernels.jl:603-668) */
jrx_status jrx_thermal2d_check_res(jrx_handle *h, const jrx_thermal2d_fields *t, const jrx_thermal2d_params *p);

/* ------------------------------------------------------------------ small backend generics of the method table
 * (src/ext/AMDGPU/3D.jl:205-239): velocity2displacement!, displacement2velocity! (types/displacement.jl:2-60), compute_dt (Utils.jl:492-519).
 * Arrays in the order x, y, z with n[d] elements each; the third pointer may be NULL in 2D. */
jrx_status jrx_velocity2displacement(jrx_handle *h, double *const U[3], const double *const V[3], const int64_t n[3], double dt);
jrx_status jrx_displacement2velocity(jrx_handle *h, double *const V[3], const double *const U[3], const int64_t n[3], double dt);
/* dt = min(dt_diff, 0.9 * min_d(di[d] / max|V_d|)); max over all ranks when a communicator is active; dt_diff = INFINITY to ignore */
jrx_status jrx_compute_dt(jrx_handle *h, const double *const V[3], const int64_t n[3], const double di[3], int32_t ndim, double dt_diff, double *dt_out);

/* ------------------------------------------------------------------ post-loop epilogue operators, stand-alone
 * The VEP drivers run these themselves (Stokes2D.jl:831-846, Stokes3D.jl:640-658); time-stepping scripts also call them directly. */
/* shear2center!(A): shear components averaged to the cell centres -- Interpolations.jl:291-323 */
jrx_status jrx_shear2center2d(jrx_handle *h, double *xy_c, const double *xy, int64_t nx, int64_t ny);
jrx_status jrx_shear2center3d(jrx_handle *h, double *yz_c, double *xz_c, double *xy_c, const double *yz, const double *xz, const double *xy,
                              int64_t nx, int64_t ny, int64_t nz);
/* accumulate_tensor!(II, A, dt): II += second_invariant_staggered(A) * dt -- StressKernels.jl:364-408 */
jrx_status jrx_accumulate_tensor2d(jrx_handle *h, double *II, const double *xx, const double *yy, const double *xy, double dt, int64_t nx, int64_t ny);
jrx_status jrx_accumulate_tensor3d(jrx_handle *h, double *II, const double *xx, const double *yy, const double *zz, const double *yz, const double *xz,
                                   const double *xy, double dt, int64_t nx, int64_t ny, int64_t nz);
/* accumulate_vol!(EVol_pl, ε_vol_pl, dt): EVol_pl += dt * ε_vol_pl over n cells -- StressKernels.jl:410-431 */
jrx_status jrx_accumulate_vol(jrx_handle *h, double *EVol, const double *evol, double dt, int64_t n);
/* compute_vorticity! as the drivers call it -- stress_rotation_particles.jl:17-50 (2D at the vertices with the velocity-node
 * spacings; 3D on the edges, forward differences at the un-shifted velocity index exactly as the reference's `_di` method) */
jrx_status jrx_compute_vorticity2d(jrx_handle *h, double *wxy, const double *Vx, const double *Vy, int64_t nx, int64_t ny, double _dx, double _dy);
jrx_status jrx_compute_vorticity3d(jrx_handle *h, double *wyz, double *wxz, double *wxy, const double *Vx, const double *Vy, const double *Vz,
                                   int64_t nx, int64_t ny, int64_t nz, double _dx, double _dy, double _dz);

/* ------------------------------------------------------------------ 3D PT heat diffusion
 * heatdiffusion_PT!(thermal, pt_thermal, thermal_bc, K, ρCp | rheology, args, dt, grid; kwargs) for 3D grids --
 * src/thermal_diffusion/DiffusionPT_solver.jl:34-149,181-305 with the 3D kernels DiffusionPT_kernels.jl:6-61,160-199,250-282.
 * Faces in the order left, right, front, back, top, bot; 3D thermal naming: bot <-> k = 1, top <-> k = end
 * (constant_value.jl:15-33) -- the opposite of the 3D velocity free-slip naming. */
typedef struct jrx_thermal3d_fields {
    double *T, *Told, *dT;                 /* (nx+2, ny+2, nz+2): thermal.T, Told, ΔT */
    double *qTx, *qTx2;                    /* (nx+1, ny, nz) */
    double *qTy, *qTy2;                    /* (nx, ny+1, nz) */
    double *qTz, *qTz2;                    /* (nx, ny, nz+1) */
    double *H, *shear_heating, *ResT;      /* ni */
    const double *K, *rhoCp;               /* ni: array-coefficient form; NULL in the rheology form */
    const double *thetar_dtau, *dtau_rho;  /* ni: PTThermalCoeffs (rewritten every iteration by jrx_heatdiffusion_PT3d_phases) */
    const double *adiabatic, *dirichlet_mask, *dirichlet_value;   /* optional, as in jrx_thermal2d_fields; mask / value (nx+2, ny+2, nz+2) */
} jrx_thermal3d_fields;

typedef struct jrx_thermal3d_params {
    int64_t nx, ny, nz;
    double _dx, _dy, _dz;
    double dt, eps;
    int64_t iterMax, nout;
    int32_t no_flux[6];
    int32_t constant_value_on[6]; double constant_value[6];
    int32_t constant_flux_on[6];  double constant_flux[6];
    int32_t periodic[6];
    int32_t rheology_form;                 /* 1: k_const, Cp, PT_Density(rho0, alpha, T0) as in test/test_diffusion3D.jl */
    double k_const, Cp, rho0, alpha, T0;
    int32_t verbose;
    double dirichlet_const;
} jrx_thermal3d_params;

jrx_status jrx_heatdiffusion_PT3d(jrx_handle *h, const jrx_thermal3d_fields *t, const jrx_thermal3d_params *p, int64_t *iter_count, double *norm_ResT,
                                  int64_t cap, int64_t *nnorms);
jrx_status jrx_thermal_bcs3d(jrx_handle *h, double *T, const jrx_thermal3d_params *p);
jrx_status jrx_thermal3d_iteration(jrx_handle *h, const jrx_thermal3d_fields *t, const jrx_thermal3d_params *p);
jrx_status jrx_thermal3d_check_res(jrx_handle *h, const jrx_thermal3d_fields *t, const jrx_thermal3d_params *p);

/* ------------------------------------------------------------------ phase-ratio form of the heat-diffusion path
 * heatdiffusion_PT!(thermal, pt_thermal, thermal_bc, rheology, args, dt, grid; kwargs = (phase = phase_ratios, ...)) --
 * src/thermal_diffusion/DiffusionPT_solver.jl:181-305 with phase !== nothing: update_pt_thermal_arrays! every iteration
 * (DiffusionPT_coefficients.jl:105-136), conductivity from the face phase ratios (DiffusionPT_kernels.jl:366-440 / :62-158), ρCp and
 * radioactive heat from the centre ratios (:553-601, :631-668 / :200-249, :283-325).  Per phase: ConstantConductivity k,
 * ConstantHeatCapacity Cp, ConstantRadioactiveHeat H_r and a density law (rho_kind as in jrx_rheology: 0 constant, 1 PT_Density,
 * 2 T_Density, 3 Compressible_Density).  p->rheology_form is ignored (set to 2 internally); t->K / t->rhoCp are not read. */
typedef struct jrx_thermal_phases {
    int32_t nphase;
    double k[JRX_MAXPHASE], Cp[JRX_MAXPHASE], Hr[JRX_MAXPHASE];
    int32_t rho_kind[JRX_MAXPHASE];
    double rho0[JRX_MAXPHASE], alpha[JRX_MAXPHASE], beta[JRX_MAXPHASE], T0[JRX_MAXPHASE], P0[JRX_MAXPHASE];
    double max_lxyz, Vpdtau;               /* pt_thermal.max_lxyz, pt_thermal.Vpdτ */
} jrx_thermal_phases;

typedef struct jrx_thermal_phase_fields {
    const double *P;                       /* args.P (ni) */
    const double *phase_c;                 /* phase_ratios.center [nphase][ni], phase index fastest */
    const double *phase_qx, *phase_qy, *phase_qz;   /* phase_ratios.Vx (nx+1, ny[, nz]), .Vy (nx, ny+1[, nz]), .Vz (nx, ny, nz+1); qz NULL in 2D */
} jrx_thermal_phase_fields;

jrx_status jrx_heatdiffusion_PT2d_phases(jrx_handle *h, const jrx_thermal2d_fields *t, const jrx_thermal2d_params *p, const jrx_thermal_phases *ph,
                                         const jrx_thermal_phase_fields *pf, int64_t *iter_count, double *norm_ResT, int64_t cap, int64_t *nnorms);
jrx_status jrx_heatdiffusion_PT3d_phases(jrx_handle *h, const jrx_thermal3d_fields *t, const jrx_thermal3d_params *p, const jrx_thermal_phases *ph,
                                         const jrx_thermal_phase_fields *pf, int64_t *iter_count, double *norm_ResT, int64_t cap, int64_t *nnorms);
/* update_pt_thermal_arrays!(pt_thermal, phase_ratios, rheology, args, _dt) -- DiffusionPT_coefficients.jl:105-136: writes thetar_dtau, dtau_rho (ni)
 * from T (ni.+2, read at Idx.+1), P and the centre ratios; n = {nx, ny, nz} (nz = 1 in 2D) */
jrx_status jrx_update_pt_thermal_arrays(jrx_handle *h, double *thetar_dtau, double *dtau_rho, const double *T, const int64_t n[3], int32_t ndim, double dt,
                                        const jrx_thermal_phases *ph, const jrx_thermal_phase_fields *pf);
/* adiabatic_heating!(thermal, stokes, rheology, phases, _dt) -- DiffusionPT_kernels.jl:720-746: A = (P - P0) * α * _dt over ncells cells, α the phase-weighted thermal
 * expansivity of the density laws (PT_Density, T_Density: α; ConstantDensity: 0 -- the values test/test_rheology.jl:57-64 asserts of get_α; Compressible_Density: 0,
 * assumed); phase_c NULL: phase 0 alone */
jrx_status jrx_adiabatic_heating(jrx_handle *h, double *adiabatic, const double *P, const double *P0, int64_t ncells, double dt, const jrx_thermal_phases *ph,
                                 const double *phase_c);

/* ------------------------------------------------------------------ grid operators of a time step, either side of solve! / heatdiffusion_PT! */
/* The methods the reference's AMDGPU extension forwards to the generic kernels (src/ext/AMDGPU/2D.jl:301-352, 3D.jl:311-362).  Shapes as in
 * StokesArrays: Vx (nx+1, ny+2[, nz+2]), Vy (nx+2, ny+1[, nz+2]), Vz (nx+2, ny+2, nz+1); shear yz (nx, ny+1, nz+1), xz (nx+1, ny, nz+1), xy (nx+1, ny+1[, nz]).
 * velocity2vertex!(Vx_v, Vy_v[, Vz_v], Vx, Vy[, Vz]) -- Interpolations.jl:212-249: the kernel runs over size(Vx_v) = (mx, my[, mz]) <= ni .+ 1 (the caller's
 *   choice, as in the reference: ni .+ 1 in the miniapps, ni in test/test_Interpolations.jl:150-164);
 * velocity2center! -- :257-289, outputs ni;
 * vertex2center!(center, vertex; ghost_x, ghost_y, ghost_z) -- :72-96: over size(vertex) .- 1, written at I .+ ghost of a centre array of extents cdim;
 * center2vertex_harm! -- :116-137 (2D, clamped harmonic mean; vertex (nx+1, ny+1));
 * center2vertex!(vertex_yz, vertex_xz, vertex_xy, center_yz, center_xz, center_xy) -- :139-178 (3D; boundary edges are not written).
 * The 2D center2vertex!(vertex, center) is jrx_center2vertex2d above. */
jrx_status jrx_velocity2vertex2d(jrx_handle *h, double *Vx_v, double *Vy_v, const double *Vx, const double *Vy, int64_t nx, int64_t ny, int64_t mx, int64_t my);
jrx_status jrx_velocity2vertex3d(jrx_handle *h, double *Vx_v, double *Vy_v, double *Vz_v, const double *Vx, const double *Vy, const double *Vz, int64_t nx,
                                 int64_t ny, int64_t nz, int64_t mx, int64_t my, int64_t mz);
jrx_status jrx_velocity2center2d(jrx_handle *h, double *Vx_c, double *Vy_c, const double *Vx, const double *Vy, int64_t nx, int64_t ny);
jrx_status jrx_velocity2center3d(jrx_handle *h, double *Vx_c, double *Vy_c, double *Vz_c, const double *Vx, const double *Vy, const double *Vz, int64_t nx,
                                 int64_t ny, int64_t nz);
jrx_status jrx_vertex2center(jrx_handle *h, double *center, const double *vertex, const int64_t vdim[3], const int64_t cdim[3], int32_t ndim, int32_t ghost_x,
                             int32_t ghost_y, int32_t ghost_z);
jrx_status jrx_center2vertex_harm2d(jrx_handle *h, double *vertex, const double *center, int64_t nx, int64_t ny);
jrx_status jrx_center2vertex3d(jrx_handle *h, double *vertex_yz, double *vertex_xz, double *vertex_xy, const double *center_yz, const double *center_xz,
                               const double *center_xy, int64_t nx, int64_t ny, int64_t nz);
/* compute_ρg!(ρg[end], [phase_ratios,] rheology, (; T, P)) -- rheology/BuoyancyForces.jl:6-60, the scalar-gravity form: rhog = density * gravity of the first
 * phase over the n = {nx, ny[, nz]} cells (the density laws of jrx_rheology; has_density must be set).  phase_c NULL: single-phase form (phase 0); T, P may be
 * NULL (= 0); P has the extents n.  tdim: the extents of args.T (NULL: n) -- T is read at the cell's own [i, j, k] of that array, so a ghosted thermal.T passed
 * as args.T is read without the shift to the centres, as the reference's getindex_NamedTuple(args, I...) does (test/test_WENO5.jl:208-214). */
jrx_status jrx_compute_rhog(jrx_handle *h, double *rhog, const jrx_rheology *rh, const double *phase_c, const double *T, const double *P, const int64_t n[3],
                            const int64_t tdim[3], int32_t ndim);
/* compute_lithostatic_pressure!(P, ρg, dz) -- src/Utils.jl:521-573: P[j] = Σ_{k>j} ρg[k] dz[k] + ρg[j] dz[j] / 2 down the columns of the last dimension (the
 * vertical, pointing up); dz_cells: one height per cell of that dimension, or NULL for the constant height dz.  n = {nx, ny[, nz]}.  The four-argument IGG
 * form (weight of the ranks stacked above) is not built: refused when the handle's communicator splits the vertical direction. */
jrx_status jrx_compute_lithostatic_pressure(jrx_handle *h, double *P, const double *rhog, double dz, const double *dz_cells, const int64_t n[3], int32_t ndim);
/* compute_viscosity!(stokes, args, rheology::MaterialParams, cutoff; relaxation = ν) -- rheology/Viscosity.jl:118-167, for the creep laws of the rheology table
 * (phase 0: LinearViscous or the Arrhenius table; they do not depend on the strain rate): eta <- clamp(ν η_creep(T, P) + (1 - ν) eta, cutoff).  args.T has the
 * extents tdim: ni .+ 2 (the ghosted thermal.T, read at I .+ 1 as local_viscosity_args does, Viscosity.jl:513-523) or ni / NULL (cell centres); P: ni or NULL.
 * The phase-ratio form is jrx_vep{2d,3d}_compute_viscosity. */
jrx_status jrx_compute_viscosity_single(jrx_handle *h, double *eta, const jrx_rheology *rh, const double *T, const double *P, const int64_t n[3],
                                        const int64_t tdim[3], int32_t ndim, double nu, double cutoff_lo, double cutoff_hi, const double *AII, int32_t tau_form);
/* AII (ni, or NULL): the invariant array of compute_viscosity_εII! / compute_viscosity_τII!(η, ν, AII, args, rheology, cutoff) (Viscosity.jl:169-196);
 * tau_form: AII is a stress invariant.  A power-law creep (visc_kind 2) needs AII here; the 2D single-material driver forms it from @strain(stokes) itself. */
/* compute_shear_heating!(thermal, stokes, [phase_ratios,] rheology, dt) -- thermal_diffusion/ShearHeating.jl:14-71:
 * shear_heating = max(0, Χ τ : (ε - ε_el)), ε_el = (τ - τ_o) / (2 G dt), at the cell centres.  tau, tau_o: @tensor_center(stokes.τ / τ_o) in Voigt order
 * (2D: xx, yy, xy_c; 3D: xx, yy, zz, yz_c, xz_c, xy_c), eps: @strain(stokes) (shear components on their edges, averaged to the centre as cache_tensors does).
 * G from rh (fn_ratio(get_shear_modulus, ...) with phase_c, phase 0 without); chi[q] = Χ of phase q's ConstantShearheating (0: no law).
 * [compute_shearheating is GeoParams': Χ Σ τ_ij (ε_ij - ε_el_ij) with the shear terms of the Voigt tuple counted twice -- form ASSUMED, parity unpinned.]
 * n = {nx, ny, nz}; ndim 2 or 3. */
jrx_status jrx_compute_shear_heating(jrx_handle *h, double *shear_heating, const double *const *tau, const double *const *tau_o, const double *const *eps,
                                     const double *phase_c, const jrx_rheology *rh, const double *chi, double dt, const int64_t n[3], int32_t ndim);

/* ------------------------------------------------------------------ WENO-5 advection (2D)
 * WENO_advection!(u, (vx, vy), weno, di, dt) -- src/advection/weno5.jl:195-230 (fluxes :10-151, weno_rhs :154-168, weno_f! :170-175; constants
 * src/types/constructors/weno.jl:7-24; AMDGPU methods src/ext/AMDGPU/2D.jl:84-88,470-472): SSP-RK3, u <- 1/3 u + 2/3 ut - 2/3 dt r(ut) with
 * ut = 3/4 u + 1/4 u1 - 1/4 dt r(u1), u1 = u - dt r(u).  method 1 = JS (Val(1)), 2 = Z (Val(2)); dx, dy the uniform spacings (_di = inv.(di)).
 * udim = size(u), vxdim / vydim = size(vx) / size(vy), wdim = the common size of weno.ut, fL, fR, fB, fT.
 * Semantics kept from the reference:
 *  - the loop box and the clamping of every stencil index come from size(u) = (nx, ny); every array is indexed with ITS OWN extents (column-major), which
 *    may be larger than u's: Benchmark2D_WENO5.jl:77,182 builds weno for ni .+ 1 and advects a field of ni, with velocities Vx_c, Vy_c larger still.  Only the
 *    (nx, ny) box of ut, fL..fT is written; the velocities are point reads vx[i, j], vy[i, j];
 *  - weno_rhs clamps iS, iN, jW, jE: on the first and last vertex of a direction the flux difference of that direction is exactly 0;
 *  - after the call weno.ut holds the stage-2 field.
 * Two kernel forms, bit-identical in u and ut (tuning key "weno_fused", include/jrx_tuning.h): the default runs one launch per RK stage with the fluxes in
 * registers, and then fL holds the stage-1 field and fR, fB, fT are not touched -- after such a call fL..fT do NOT hold fluxes (nothing outside weno5.jl
 * reads them); "weno_fused" = 0 runs the reference's six launches and leaves the fluxes of the stage-2 field in fL..fT.  3D fields: jrx_weno5_advection3d
 * below (the reference's 3D forwards, src/ext/AMDGPU/3D.jl:71-75,493-495, feed a 3D array into this 2D indexing).  No halo exchange (the reference has none; callers update_halo!).
 * JRX_ERR_ARG without a launch: method not 1 or 2, nx or ny < 1, any of vx, vy, ut, fL..fT smaller than u along a dimension, two arrays overlapping (vx, vy
 * excepted).  JRX_ERR_UNSUPPORTED: an array of 2^31 or more entries (32-bit offsets).  Counters "stat_weno_calls", "stat_weno_fused" (jrx_get_option). */
jrx_status jrx_weno5_advection2d(jrx_handle *h, double *u, const int64_t udim[2], const double *vx, const int64_t vxdim[2], const double *vy,
                                 const int64_t vydim[2], double *ut, double *fL, double *fR, double *fB, double *fT, const int64_t wdim[2], double dx, double dy,
                                 double dt, int32_t method);

/* ------------------------------------------------------------------ WENO-5 advection (3D)
 * WENO_advection!(u, (vx, vy, vz), weno, di, dt) on a 3D vertex field: jrx_weno5_advection2d one dimension up.  The reference defines the scheme one direction
 * at a time (src/advection/weno5.jl:10-168) but its 3D methods (src/ext/AMDGPU/3D.jl:71-75,493-495) feed a 3D array into the 2D indexing, so the 3D form is
 * written out here: the same clamped five-point reconstruction along z, two more terms in weno_rhs, the same SSP-RK3.  method, dt as in 2D; dx, dy, dz the
 * uniform spacings.  udim = size(u), vxdim / vydim / vzdim = size(vx) / size(vy) / size(vz), wdim = the common size of weno.ut and the six flux arrays.
 *  - the loop box and the clamping of every stencil index come from size(u) = (nx, ny, nz); every array is indexed with ITS OWN extents (column-major), which
 *    may be larger than u's.  Only the (nx, ny, nz) box of ut and the flux arrays is written; the velocities are point reads vx[i, j, k], vy[i, j, k], vz[i, j, k];
 *  - fB / fT are the upwind / downwind fluxes along x and fL / fR those along y, as in the reference; fD / fU are the upwind / downwind fluxes along z (from
 *    u[i, j, k-2..k+2]) -- these two names are this project's, the reference's struct has no such fields;
 *  - weno_rhs = the reference's four terms followed by max(vz,0) (fD[i,j,k] - fD[i,j,kD]) _dz + min(vz,0) (fU[i,j,kU] - fU[i,j,k]) _dz with kD = clamp(k-1),
 *    kU = clamp(k+1): on the first and last vertex of a direction the flux difference of that direction is exactly 0 (the reference's quirk, kept).  The device
 *    evaluates the z terms first (innermost), then the y and x chain of the 2D kernels: for a field constant along z the result has the 2D entry point's bits;
 *  - after the call weno.ut holds the stage-2 field.
 * Two kernel forms, bit-identical in u and ut (tuning key "weno_fused"): the default runs one launch per RK stage with the fluxes in registers and LDS; then fL
 * holds the stage-1 field and fR, fB, fT, fD, fU are not touched and may be NULL.  "weno_fused" = 0 runs six launches and leaves the six fluxes of the stage-2
 * field; all six flux arrays must then be non-NULL.  No halo exchange, as in 2D.
 * JRX_ERR_ARG without a launch: method not 1 or 2, an extent of u < 1, any of vx, vy, vz, ut and the flux arrays smaller than u along a dimension, two arrays
 * overlapping (the velocities among themselves excepted), a NULL flux array with "weno_fused" = 0.  JRX_ERR_UNSUPPORTED: an array of 2^31 or more entries
 * (32-bit offsets).  Counters "stat_weno3d_calls", "stat_weno3d_fused" (jrx_get_option); the 2D counters count 2D calls only. */
jrx_status jrx_weno5_advection3d(jrx_handle *h, double *u, const int64_t udim[3], const double *vx, const int64_t vxdim[3], const double *vy,
                                 const int64_t vydim[3], const double *vz, const int64_t vzdim[3], double *ut, double *fL, double *fR, double *fB, double *fT,
                                 double *fD, double *fU, const int64_t wdim[3], double dx, double dy, double dz, double dt, int32_t method);

/* ------------------------------------------------------------------ principal stresses
 * compute_principal_stresses!(stokes, σ) -- src/stokes/PrincipalStresses.jl:1-63 (hessenberg_eigen_3x3 :67-97), PrincipalStress
 * src/types/constructors/stokes.jl:121-147, AMDGPU methods src/ext/AMDGPU/2D.jl:182-197, 3D.jl:187-202.  Inputs are @stress_center(stokes.τ)
 * (src/Utils.jl:346-355), (nx, ny[, nz]) = size(stokes.P); outputs s1, s2[, s3] are (2, nx, ny) / (3, nx, ny, nz) arrays, column-major with the component
 * index fastest (σ.σ1[i, I...]).  One launch, synchronous.
 *  - 2D: the reference's closed form KEPT AS WRITTEN (PrincipalStresses.jl:20-36), so that one script gives the same numbers on every backend:
 *    a = (xx + yy)/2, b = sqrt((xx - yy)^2/2 + xy^2) -- /2 where the eigenvalues need /4, so diag(1, -1) gives +-sqrt(2) --, s1 = (a + b)(cos t, sin t),
 *    s2 = (a - b)(-sin t, cos t) with t = atan(2 xy / (xx - yy))/2, the one-argument atan: where xx < yy, s1 lies along the minor axis; where xx = yy and
 *    xy = 0 the vectors are NaN (0/0).  The (2, 1, 1) placeholder σ.σ3 is not passed and never written.
 *  - 3D: a DELIBERATE DEVIATION: the exact eigendecomposition instead of hessenberg_eigen_3x3, whose QR steps shifted by H[3,3] with an absolute tolerance
 *    of 1e-10 and at most 50 iterations cannot split +-s of a simple shear (it returns (0, 0, 0) there) and never meet the tolerance at Pa-scale stresses.
 *    Where the reference converges the two agree (its own case xx, yy, zz = 1, 2, 3, xy, xz, yz = .5, .25, .75 gives 3.48702452, 1.721857, 0.79111848).
 *    s_j = lambda_j e_j with lambda_1 >= lambda_2 >= lambda_3 (signed, as reverse(sortperm(σ))), e_j a unit eigenvector whose largest-magnitude component
 *    is positive (the lowest index on ties); a zero tensor gives zeros; a NaN / Inf cell gives non-finite output for that cell only.  Cyclic Jacobi in
 *    fp64 registers, a fixed cap on the sweeps.
 * JRX_ERR_ARG without a launch: a NULL pointer, an extent < 1, overlapping outputs or an output overlapping an input.  JRX_ERR_UNSUPPORTED: 2^39 or more
 * cells.  Counter "stat_principal_calls" (jrx_get_option) counts the calls that launched. */
jrx_status jrx_principal_stresses2d(jrx_handle *h, double *s1, double *s2, const double *xx, const double *yy, const double *xy_c, int64_t nx, int64_t ny);
jrx_status jrx_principal_stresses3d(jrx_handle *h, double *s1, double *s2, double *s3, const double *xx, const double *yy, const double *zz,
                                    const double *yz_c, const double *xz_c, const double *xy_c, int64_t nx, int64_t ny, int64_t nz);

/* ------------------------------------------------------------------ phase ratios from phase fields
 * update_phase_ratios_2D!(phase_ratios, phase_arrays, xci, xvi) / update_phase_ratios_3D!(...) -- src/phases/PhaseRatios.jl:24-35 / :61-78 (centres :89-116,
 * vertices :135-211, faces :231-293, edges :324-383): the particle-free route to a PhaseRatios -- advect N cell-centred phase fields (values nominally in
 * [0, 1]), then rebuild every member from them.  phase_arrays is a HOST array of nphase DEVICE pointers to (nx, ny[, nz]) arrays; xc[d] / xv[d] are device
 * pointers to the n_d cell centres / n_d + 1 vertices of dimension d; dx[d] = xv[d][1] - xv[d][0] (compute_dx needs ranges: the grid is uniform).  Outputs in
 * CellArray layout, the phase index fastest: center (N, ni...), vertex (N, ni .+ 1 ...), Vx (N, nx+1, ny[, nz]), Vy, Vz and in 3D the edges yz (N, nx, ny+1, nz+1),
 * xz (N, nx+1, ny, nz+1), xy (N, nx+1, ny+1, nz).  Rules kept from the reference, operation for operation:
 *  - every member accumulates w_k += weight * p_k[cell], W += weight over its cells, skipping the cells outside the grid, then applies one tail, every sum over
 *    k = 1..N left to right: w_k / W; clamp to [0, 1]; values < 1e-5 become 0; s = sum; write w_k / s.  Centres: w_k = p_k[I] divided by t = sum of p_k[I];
 *  - faces: the cells I_d - 1, then I_d across the face, weight 0.5 each (a boundary face has W = 0.5); edges: the four cells at offsets (-1,-1), (-1,0),
 *    (0,-1), (0,0) in (first, second staggered dimension), weight 0.25 each;
 *  - vertices: the 2^ndim cells at offsets {-1, 0}, the first dimension's offset outermost, -1 before 0; 2D weight wx wy with
 *    wx = fma(-|xv_1[i] - xc_1[ic]|, 1/dx_1, 1) (the reference's muladd), 3D weight ((1 - |xv_1 - xc_1| (1/dx_1)) (1 - ...)) (1 - ...) without fma.  The weights
 *    come from the coordinates passed in, not from an assumed 0.5;
 *  - a cell whose arrays sum to 0, or that holds a NaN, gives NaN for every phase at exactly the nodes that read it.
 * Two kernel forms with identical bits in every member (tuning key "phase_ratios_fused", include/jrx_tuning.h): the default is ONE launch, a thread per node
 * of the ni .+ 1 box that reads its 2^ndim cells once and writes every member it owns; 0 runs one launch per member (4 in 2D, 8 in 3D).  No halo exchange
 * (the reference has none).  Synchronous.
 * JRX_ERR_ARG without a launch, with a text naming the cause: a NULL pointer (an entry of phase_arrays, xc, xv included), nphase outside 1..JRX_MAXPHASE, an
 * extent < 1, a dx that is not positive and finite, an output overlapping an input or another output.  JRX_ERR_UNSUPPORTED: an output of 2^31 or more entries
 * (32-bit offsets).  Counters "stat_phase_ratios_calls" / "stat_phase_ratios_fused" (jrx_get_option). */
jrx_status jrx_update_phase_ratios2d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *const *phase_arrays, int32_t nphase,
                                     int64_t nx, int64_t ny, const double *const xc[2], const double *const xv[2], const double dx[2]);
jrx_status jrx_update_phase_ratios3d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, double *Vz, double *yz, double *xz, double *xy,
                                     const double *const *phase_arrays, int32_t nphase, int64_t nx, int64_t ny, int64_t nz, const double *const xc[3],
                                     const double *const xv[3], const double dx[3]);

/* ------------------------------------------------------------------ grid-based stress rotation and advection
 * rotate_stress!(stokes, grid, dt; method, advection) on grids: carries stokes.τ to stokes.τ_o through one time step -- rotated by the vorticity (Jaumann rate)
 * and advected by the velocity -- where every driver's epilogue leaves a plain copy.  The reference does this on particles (rotate_stress!(pτ, stokes,
 * particles, dt) then stress2grid!, src/stress_rotation/stress_rotation_particles.jl:205-299); it also exports a grid form, rotate_stress!(V, τ, _di, dt),
 * src/stress_rotation/stress_rotation_grid.jl, which is the counterpart built here.  That text is a stub and is NOT restated.  Its defects, not followed:
 *  - :68 multiplies the advective term by 0 and overwrites the stress with τR - Rτ (:54-63): no dt, and the old stress is gone;
 *  - advection_term (:157-168) takes the downwind difference (Vx > 0 ? dx_right : dx_left);
 *  - upwind_derivatives (:115-154) replaces the neighbour of the second and of the last-but-one row by 0 (i - 1 > 1, i + 1 < nx);
 *  - it writes τ in place while other threads read the neighbours;
 *  - the "3D" method calls rotate_elastic_stress2D and the 2D matrices, and tensor2voigt (:16-24) indexes 3D arrays with two indices;
 *  - its Jaumann sibling on particles (stress_rotation_particles.jl:151-167) adds +2 dt ω τxy to both xx and yy, which changes the trace; the rate is
 *    -2 dt ω τxy on xx and +2 dt ω τxy on yy.
 * Kept from the reference: the per-point rotation-matrix form rotate_stress_particles_rotation_matrix! (stress_rotation_particles.jl:169-201), the ω
 * convention of compute_vorticity! (:17-80; jrx_compute_vorticity2d / 3d) and velocity2center (stress_rotation_grid.jl:171-176).
 *
 * Definition (uniform grids; indices 1-based).  One explicit step, out of place, both terms from the input state:
 *     τ_o[c](I) = Rot_c(τ, ω dt)(I) - dt Adv(τ[c], v)(I)        for every member c at its own node I.
 * Members.  2D, tau / tau_o = {xx, yy, xy_c (centres, ni), xy (vertices, ni .+ 1), xx_v, yy_v (vertices; optional: all four pointers or they are skipped)}.
 * 3D, tau / tau_o = {xx, yy, zz, yz_c, xz_c, xy_c (centres), yz (nx, ny+1, nz+1), xz (nx+1, ny, nz+1), xy (nx+1, ny+1, nz)}.  The _c members are inputs as the
 * drivers leave them, not rebuilt from the edges.  ω: 2D omega_xy (ni .+ 1); 3D omega = {yz, xz, xy} on the edge arrays.  V = {Vx, Vy[, Vz]} with ghost layers.
 * Interpolation.  A quantity that does not live at the target node is the mean of the 2^m nearest nodes of its own array, m = the number of axes along which
 * the two locations are half a cell apart: indices clamped into the source's extent, the 2^m values summed in index order (x fastest), times 1 / 2^m.  So the
 * normals at a vertex / edge come from 4 centres, ω at a centre from 4 vertices / edges, a foreign shear or ω component at an edge from 4 nodes of the other
 * edge family; the 2D xx_v, yy_v are rotated from their own node (xx_v, yy_v, xy) without interpolation.  Velocities alike, every node existing thanks to
 * the ghost layers: 2D centre vx = ½(Vx[i,j+1] + Vx[i+1,j+1]), vy = ½(Vy[i+1,j] + Vy[i+1,j+1]); 2D vertex vx = ½(Vx[i,j] + Vx[i,j+1]), vy = ½(Vy[i,j] +
 * Vy[i+1,j]); 3D: 2 nodes for the in-plane components of an edge, 8 for the one normal to its plane.
 * Rotation.  JRX_ROTATE_MATRIX: 2D θ = dt ω, τ' = R (τ R') with R = [c -s; s c], multiplied out in the order of :182-197.  3D: the axial vector
 * w = (ω_yz, ω_xz, ω_xy) (half the curl), θ = dt |w|, n = w / |w|, R = I + sinθ K + (1 - cosθ) K², K = [n]x, τ' = R (τ R'); |w| == 0 gives R = I without a
 * division.  JRX_ROTATE_JAUMANN: τ' = τ + dt (W τ - τ W), W = [w]x; in 2D xx - 2θ xy, yy + 2θ xy, xy + θ (xx - yy).
 * Advection.  JRX_ADVECT_UPWIND: Adv(A, v)(I) = Σ_d v_d (v_d > 0 ? A[I] - A[I - e_d] : A[I + e_d] - A[I]) _d_d, a neighbour outside the array replaced by A[I].
 * JRX_ADVECT_NONE: the term is not evaluated and V (or its entries) may be NULL.  There is no CFL check: dt must come from compute_dt.  compute_dt bounds the
 * Courant number of each axis by 0.9; the unsplit upwind step is stable while their SUM over the axes stays <= 1 at every node, so a flow whose components reach
 * their maxima at the same nodes (the corners of a box in solid-body rotation) needs compute_dt / ndims (examples/stress_rotation2d.py).
 * No fma anywhere: every product and sum is rounded once in the order stated (tests/_stress_rotation.py is the same text in NumPy).  One launch, a thread per
 * node of the ni .+ 1 box writes every member that node owns.  No halo exchange inside the call.  Synchronous.  Counter "stat_rotate_stress_calls".
 * tau_o, tau, omega, V are HOST arrays of DEVICE pointers.  JRX_ERR_ARG (4) with a text naming the cause, nothing launched and nothing written: an output
 * that overlaps an input (or another output), a NULL required member, an unknown method or advection kind, an extent < 1, 2^31 or more entries in the
 * ni .+ 2 box that holds every array (32-bit offsets). */
#define JRX_ROTATE_MATRIX 0
#define JRX_ROTATE_JAUMANN 1
#define JRX_ADVECT_NONE 0
#define JRX_ADVECT_UPWIND 1
jrx_status jrx_rotate_stress2d(jrx_handle *h, double *const tau_o[6], const double *const tau[6], const double *omega_xy, const double *const V[2], int64_t nx,
                               int64_t ny, const double _di[2], double dt, int32_t method, int32_t advection);
jrx_status jrx_rotate_stress3d(jrx_handle *h, double *const tau_o[9], const double *const tau[9], const double *const omega[3], const double *const V[3],
                               int64_t nx, int64_t ny, int64_t nz, const double _di[3], double dt, int32_t method, int32_t advection);

/* ------------------------------------------------------------------ a moving free surface in 2D: topography field, rock fractions from it
 * The variational drivers take a RockRatio; jrx_update_rock_ratio derives one from the air phase's ratios, so the surface sits where the advected air field
 * happens to be smeared.  These three operators track the surface itself: a height field h at the nx + 1 vertex abscissae (Python: Topography(backend, nx),
 * members h and h_old), the rock fractions from it, its advection and the phase correction.  NO reference text exists to restate: the reference's free-surface
 * miniapps (miniapps/DYREL2D/volcano/Caldera2D.jl:175-195,439-449 and the Subduction2D_VS* set) call JustPIC's marker chain -- fill_chain_from_vertices!,
 * semilagrangian_advection_markerchain!, compute_rock_fraction!(ϕ, chain, xvi, di) -- which is not in the reference tree, and update_phases_given_markerchain!
 * (src/phases/topography_correction.jl:64-90, with its closest_phase) works on particles.  What is built is defined here, to the rounding.
 *
 * Scope: 2D, uniform grid, one block.  fp64, no fma anywhere (the library builds with -ffp-contract=off): every product and sum is rounded once, left to right as
 * written, so tests/_topography.py (the same text in NumPy) agrees bit for bit.  Indices 0-based, x fastest; ni = (nx, ny), y0 the grid's origin in y, _dx, _dy the
 * inverse spacings.  The surface is the polyline through (x_v[i], h[i]).
 *   clamp(x, lo, hi) = x >= lo ? (x <= hi ? x : hi) : lo      (comparisons; a NaN becomes lo)
 *   s[i] = (h[i] - y0) * _dy                                    heights in cell units
 *   m[i] = 0.5 * (s[i] + s[i+1])                                midpoint of segment i
 *   Φ(g) = 0 for g <= 0;  (0.5 * g) * g for 0 < g < H;  H * g - (0.5 * H) * H for g >= H
 *   P(ga, gb, w, H): one linear piece with end heights ga, gb above the bottom of a volume of width w and height H (cell units):
 *       ga == gb:  w * clamp(ga, 0, H);      otherwise:  (w * (Φ(gb) - Φ(ga))) / (gb - ga)
 *   Volumes centred on a vertex row j:  b = max(j - 0.5, 0), t = min(j + 0.5, ny), H = t - b  (clipped to the domain, normalised by what remains).
 *
 * 1. compute_rock_fraction!(ϕ::RockRatio, topo, grid) -- jrx_compute_rock_fraction2d.  Writes all four 2D members of ϕ, each the fraction of the member's
 *    control volume below the polyline:
 *      center[i,j] (nx, ny)        P(s[i]-j, s[i+1]-j, 1, 1)
 *      Vy[i,j]     (nx, ny+1)      P(s[i]-b, s[i+1]-b, 1, H) / H
 *      Vx[i,j]     (nx+1, ny)      ( left half P(m[i-1]-j, s[i]-j, 0.5, 1) if i > 0, + right half P(s[i]-j, m[i]-j, 0.5, 1) if i < nx, added in that order ) / W
 *      vertex[i,j] (nx+1, ny+1)    the two halves of Vx with b, H of Vy, divided by (W * H)
 *    W = the width present, 1 or 0.5.  Every value is finally passed through clamp(., 0, 1): a guarantee for the masks of the solver (isvalid is `> 0`); no input
 *    has been found for which the quotient leaves [0, 1].  One launch, a thread per node of the ni .+ 1 box writes every member that node owns; the only loads are
 *    h[i-1], h[i], h[i+1].  Nothing else in ϕ is read.
 *    Against jrx_update_rock_ratio on binary phase fields with the air above a face-aligned surface: center is bit-identical.  That operator interpolates ratios and this one
 *    integrates areas, so the other members need not agree; on that flat surface they do (largest difference measured over vertex, Vx, Vy: 0 -- the interpolated
 *    ratio of the face row is 0.5, the area fraction of its volume; tests/test_topography_restatement.py prints it).  Under a sloped or mid-cell surface the two
 *    routes answer different questions and no agreement is claimed.
 * 2. advect_topography!(topo, V, grid, dt) -- jrx_advect_topography2d.  V = (Vx (nx+1, ny+2), Vy (nx+2, ny+1)) as stokes.V, with ghost layers.  The call copies
 *    h to h_old, then writes every h[i] from h_old (s_old its heights in cell units):
 *      vertex velocities (as for the stress rotation above):  vxv(i,j) = 0.5 * (Vx[i,j] + Vx[i,j+1]),  vyv(i,j) = 0.5 * (Vy[i,j] + Vy[i+1,j])
 *      surface velocity at the arrival point:  σ = clamp(s_old[i], 0, ny), j0 = min(floor(σ), ny - 1), t = σ - j0,  v = (1 - t) * v(i,j0) + t * v(i,j0+1) for vx, vy
 *      departure point:  ξ = clamp(i - (vx * dt) * _dx, 0, nx), i0 = min(floor(ξ), nx - 1), r = ξ - i0
 *      new height:  h[i] = ((1 - r) * h_old[i0] + r * h_old[i0+1]) + vy * dt
 *    First order, unconditionally stable; dt comes from compute_dt undivided (the two Courant numbers need not sum below 1 as for the upwind step above).
 *    The step has no limit of its own, but a time loop with a free surface has one: compute_dt is 0.9 d / max|V| and the velocities shrink as the surface
 *    flattens, so the Courant step outgrows the relaxation time 4 π η / (ρ g λ) of the longest wavelength and the explicit update then overshoots
 *    (examples/free_surface_relaxation2d.py passes a quarter of that time as the dt_diff of compute_dt).
 * 3. update_phases_given_topography!(phases, topo, grid, air_phase) -- jrx_update_phases_topography2d.  phases: the N cell-centred (nx, ny) phase fields that
 *    update_phase_ratios_2D! takes, 1 <= N <= JRX_MAXPHASE, a HOST array of DEVICE pointers; air_phase is 1-based.  A thread per column marches j = 0 .. ny - 1
 *    and carries rock proportions p_k (k over the non-air indices; before any cell with rock: 1 on the lowest non-air index, 0 elsewhere).  In each cell, with
 *    c_k the fields' values, f = center[i,j] of operator 1 (computed in the kernel) and R = the sum of the non-air c_k in index order:
 *      if R > 0:  p_k = c_k / R  (else the carried set stays);
 *      if c_air == 1 - f the cell is left untouched;  otherwise  c_k = f * p_k  for the non-air k and  c_air = 1 - f.
 *    Air below the surface becomes the nearest rock below it, rock above the surface becomes air (the grid counterpart of closest_phase).
 *
 * All three are synchronous.  JRX_ERR_ARG (4) with a text naming the cause, nothing launched and no counter moved: a NULL member, an extent < 1, air_phase
 * outside 1..N, N outside 1..JRX_MAXPHASE, overlapping outputs (or an output that overlaps an input), 2^31 or more entries in the ni .+ 2 box that holds every
 * array (32-bit offsets), a non-finite dt, _dx, _dy or y0. */
jrx_status jrx_compute_rock_fraction2d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *topo_h, int64_t nx, int64_t ny,
                                       double y0, double _dy);
jrx_status jrx_advect_topography2d(jrx_handle *h, double *topo_h, double *topo_h_old, const double *Vx, const double *Vy, int64_t nx, int64_t ny, double y0,
                                   double _dx, double _dy, double dt);
jrx_status jrx_update_phases_topography2d(jrx_handle *h, double *const *phases, int32_t nphase, const double *topo_h, int64_t nx, int64_t ny, double y0,
                                          double _dy, int32_t air_phase);

/* ------------------------------------------------------------------ a moving free surface in 3D: topography h(x, y), rock fractions from it
 * The 3D forms of the three operators above, for the eight-member RockRatio of the 3D variational driver (Python: Topography(backend, (nx, ny)), h and h_old of
 * shape (nx+1, ny+1)).  As in 2D there is no reference text to restate (JustPIC's marker chain is not in the reference tree); what is built is defined here, to
 * the rounding.  Scope: 3D, uniform grid, one block.  fp64, no fma: every product and sum is rounded once, left to right as written, so tests/_topography3d.py
 * (the same text in NumPy) agrees bit for bit.  Indices 0-based, x fastest; ni = (nx, ny, nz), z the vertical, z0 the grid's origin in z, _dx, _dy, _dz the
 * inverse spacings; clamp as above.
 *
 * The surface.  Heights h[i,j] at the (nx+1) x (ny+1) vertex positions; s[i,j] = (h[i,j] - z0) * _dz in cell units; every cell (i,j) has the centre value
 *   c[i,j] = 0.25 * ((s[i,j] + s[i+1,j]) + (s[i,j+1] + s[i+1,j+1]))
 * and is split into the four triangles corner-corner-centre, the surface linear on each: no diagonal bias, and on a surface constant along y the 2D polyline.
 * A QUADRANT is the quarter of cell (i,j) at one of its corners: two half-triangles of area 1/8 with the vertex values (A, mx, c) and (A, my, c), A the corner's
 * height, X and Y the heights of the cell's neighbouring corners along x and y, mx = 0.5 * (A + X), my = 0.5 * (A + Y).
 * The mean over a triangle of clamp(g, 0, H), g linear with the vertex values g1, g2, g3 sorted to a <= b <= c (three comparisons):
 *   Ψ(a,b,c) = 0                                                    if c <= 0
 *            = ((a + b) + c) / 3                                     if a >= 0
 *            = ((c * c) * c) / ((3 * (c - a)) * (c - b))              if b <= 0
 *            = ((a + b) + c) / 3 + (((-a) * (-a)) * (-a)) / ((3 * (b - a)) * (c - a))      otherwise
 *   T(g1,g2,g3,H) = H if a >= H;  0 if c <= 0;  otherwise Ψ(a, b, c) - Ψ(a - H, b - H, c - H)
 * The two shortcuts of T are part of the definition: a fully covered volume is exactly 1, and a kernel may skip the arithmetic without changing a bit.
 * A quadrant's volume inside the z range [b, b + H]:
 *   q = 0.125 * T(A - b, mx - b, c - b, H) + 0.125 * T(A - b, my - b, c - b, H)
 *
 * 1. compute_rock_fraction!(ϕ::RockRatio{3}, topo, grid) -- jrx_compute_rock_fraction3d.  Writes all eight members of ϕ, each the fraction of the member's
 *    control volume below the surface.  Four footprints, built from quadrants named by the vertex they touch and the direction (+-x, +-y); their volumes are
 *    added in the order listed, starting from 0; a quadrant whose cell is outside the domain is skipped:
 *      cell (i,j):                 (i,j,+,+), (i+1,j,-,+), (i,j+1,+,-), (i+1,j+1,-,-)                                   area 1
 *      x-face (i,j), i = 0..nx:    (i,j,-,+), (i,j+1,-,-) if i > 0; then (i,j,+,+), (i,j+1,+,-) if i < nx                area 1 or 0.5
 *      y-face (i,j), j = 0..ny:    (i,j,+,-), (i+1,j,-,-) if j > 0; then (i,j,+,+), (i+1,j,-,+) if j < ny                area 1 or 0.5
 *      vertex (i,j):               (-,-), (+,-), (-,+), (+,+) of the vertex, those that exist                          area 0.25 * their number
 *    Two z ranges:  cell row k: b = k, H = 1;   vertex row k: b = max(k - 0.5, 0), t = min(k + 0.5, nz), H = t - b.
 *      center (nx, ny, nz)      cell, cell row        Vz (nx, ny, nz+1)        cell, vertex row
 *      Vx (nx+1, ny, nz)        x-face, cell row      xz (nx+1, ny, nz+1)      x-face, vertex row
 *      Vy (nx, ny+1, nz)        y-face, cell row      yz (nx, ny+1, nz+1)      y-face, vertex row
 *      xy (nx+1, ny+1, nz)      vertex, cell row      vertex (nx+1, ny+1, nz+1) vertex, vertex row
 *    On a surface constant along y the y-face members equal their cell partners bit for bit on interior rows (the same volumes in the same order); the vertex
 *    footprint adds the volumes of the x-face in another order, and a footprint clipped at a face of the domain has half of them, so those pairs (and every
 *    pair after x and y are exchanged) agree only to the rounding of the sum.
 *    The value is clamp(sum / (area * H), 0, 1): as in 2D a guarantee for the masks of the solver (the sum itself is good to a few 1e-16).  One launch; the only loads are the nine heights around (i,j); nothing
 *    else in ϕ is read.  A thread owns a node (i,j) of the (nx+1, ny+1) vertex positions and a chunk of vertex rows k (tuning key "rock_fraction3d_rows",
 *    include/jrx_tuning.h); a row whose z range lies below the smallest (above the largest) of the nine heights is 1 (0) by the shortcuts, the others are evaluated.
 * 2. advect_topography!(topo, V, grid, dt) -- jrx_advect_topography3d.  V = stokes.V with ghost layers: Vx (nx+1, ny+2, nz+2), Vy (nx+2, ny+1, nz+2),
 *    Vz (nx+2, ny+2, nz+1).  The call copies h to h_old, then writes every h[i,j] from h_old (s_old its heights in cell units).  Vertex velocities, paired so
 *    that a plane-strain state reproduces the bits of the 2D operator:
 *      vxv(i,j,k) = 0.25 * ((Vx[i,j,k] + Vx[i,j,k+1]) + (Vx[i,j+1,k] + Vx[i,j+1,k+1]))
 *      vyv(i,j,k) = 0.25 * ((Vy[i,j,k] + Vy[i,j,k+1]) + (Vy[i+1,j,k] + Vy[i+1,j,k+1]))
 *      vzv(i,j,k) = 0.25 * ((Vz[i,j,k] + Vz[i+1,j,k]) + (Vz[i,j+1,k] + Vz[i+1,j+1,k]))
 *      at the surface:  σ = clamp(s_old[i,j], 0, nz), k0 = min(floor(σ), nz - 1), t = σ - k0,  v = (1 - t) * v(i,j,k0) + t * v(i,j,k0+1) for vx, vy, vz
 *      departure point: ξ = clamp(i - (vx * dt) * _dx, 0, nx), i0 = min(floor(ξ), nx - 1), r = ξ - i0;  η = clamp(j - (vy * dt) * _dy, 0, ny), j0 = min(floor(η), ny - 1), q = η - j0
 *      h[i,j] = ((1 - q) * ((1 - r) * h_old[i0,j0] + r * h_old[i0+1,j0]) + q * ((1 - r) * h_old[i0,j0+1] + r * h_old[i0+1,j0+1])) + vz * dt
 *    First order, stable at any dt.  The 2D remark about the relaxation time applies unchanged, and weighs more: the 3D variational driver has no free-surface
 *    stabilisation (examples/free_surface_relaxation3d.py passes a quarter of that time as the dt_diff of compute_dt).
 * 3. update_phases_given_topography!(phases, topo, grid, air_phase) -- jrx_update_phases_topography3d.  phases: the N cell-centred (nx, ny, nz) fields that
 *    update_phase_ratios_3D! takes, 1 <= N <= JRX_MAXPHASE, a HOST array of DEVICE pointers; air_phase is 1-based.  A thread per column (i,j) marches
 *    k = 0 .. nz - 1 by exactly the 2D rule, with f = center[i,j,k] of operator 1 computed in the kernel.
 *
 * All three are synchronous and count in the 2D operators' counters.  JRX_ERR_ARG (4) with a text naming the cause, nothing launched and no counter moved: a NULL
 * member, an extent < 1, air_phase outside 1..N, N outside 1..JRX_MAXPHASE, overlapping outputs (or an output that overlaps an input), 2^31 or more entries in the
 * ni .+ 2 box, a non-finite dt, spacing or z0. */
jrx_status jrx_compute_rock_fraction3d(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, double *Vz, double *yz, double *xz, double *xy,
                                       const double *topo_h, int64_t nx, int64_t ny, int64_t nz, double z0, double _dz);
jrx_status jrx_advect_topography3d(jrx_handle *h, double *topo_h, double *topo_h_old, const double *Vx, const double *Vy, const double *Vz, int64_t nx, int64_t ny,
                                   int64_t nz, double z0, double _dx, double _dy, double _dz, double dt);
jrx_status jrx_update_phases_topography3d(jrx_handle *h, double *const *phases, int32_t nphase, const double *topo_h, int64_t nx, int64_t ny, int64_t nz, double z0,
                                          double _dz, int32_t air_phase);

/* ------------------------------------------------------------------ timing hooks for bench.py */
/* Runs `iters` PT iterations of the 3D loop body back to back (no norm checks) and reports device times
 * measured with hipEvents on the handle's stream inside that batch:
 *   times_ms[0] whole batch; [1] mean stand-alone stress sweep; [2] mean stand-alone velocity sweep;
 *   [3] mean fused launch group (k_fused3d = velocity sweep m + BCs + stress sweep m+1, then the ghost-plane and
 *   boundary-plane launches), 0 when nothing was fused; [4] mean k_fused3d launch alone (without neighbours: the launch over the
 *   interior tiles, while the high-face tiles and the boundary layers run beside it on the halo stream); [5] the number of cells
 *   whose stresses the launch timed in [4] updates (its units; 0 when nothing was fused). */
jrx_status jrx_stokes3d_iterate_timed(jrx_handle *h, const jrx_stokes3d_fields *f, const double *etatau,
                                      const jrx_stokes3d_params *p, int64_t iters, double times_ms[6]);

/* ------------------------------------------------------------------ 2D DYREL: self-tuned dynamic relaxation inside Powell-Hestenes pressure iterations
 * solve_DYREL!(stokes, ρg, dyrel, flow_bcs, phase_ratios, rheology, args, grid, dt, igg; kwargs...) -- src/DYREL/solver.jl:44-294 (_solve_DYREL!), with
 * DYREL / DYREL! (src/DYREL/types.jl:24-59, constructors.jl:13-57,137-190), the table rheology of jrx_rheology (every visc_kind, ConstantElasticity, an optional
 * DruckerPrager_regularised with the softening laws, the density laws for compute_ρg! / update_ρg!) and both values of linear_viscosity.
 * Built: 2D, one block, uniform spacing, velocity boundary conditions (free slip / no slip), the plain pressure residual -∇V - (P - P0)/ηb + Q/dt.
 * Status JRX_ERR_ARG before anything is launched, with a text that names the cause, for: a handle with a communicator; p->inv_spacing non-NULL; a RockRatio
 * (phi non-NULL: the ϕ methods of constructors.jl:192,259, stress_kernels.jl:320-431, velocity_kernels_VS.jl); an is_pl other than 0 or 1; the thermal and
 * melt-fraction forms of _RP_cell (pressure_kernels.jl:54-127: d->dT or d->melt_fraction non-NULL); periodic faces; 2^31 or more entries in an array.
 * Of jrx_vep2d_params these entry points read nx, ny, nxg, nyg, _dx, _dy (= inv(dx), inv(dy): Gershgorin.jl:47-48 inverts the same spacing), dt, free_slip,
 * no_slip, periodic, T_ghosted and inv_spacing; the solver's keywords are jrx_dyrel2d_params.  Counter "stat_dyrel_launches" (jrx_get_option): kernels launched
 * by these entry points.
 * jrx_dyrel2d_fields: the arrays of the DYREL struct a 2D solve uses (types.jl:24-59 less the 3D members Dz, λmaxVz, dVzdτ, dτVz, dVz, βVz, cVz, αVz, Rz0):
 * γ_eff, ηb, P_num (ni); Dx, λmaxVx, dVxdτ, dτVx, dVx, βVx, cVx, αVx, Rx0 (nx-1, ny) and their y members (nx, ny-1); then the StokesArrays members that
 * jrx_vep2d_fields does not carry: τ.xx_v, τ.yy_v, τ_o.xx_v, τ_o.yy_v, λv (ni .+ 1), λ, ΔPψ (ni); then args.ΔT and args.melt_fraction, which must be NULL. */
typedef struct jrx_dyrel2d_fields {
    double *gamma_eff, *etab, *P_num;
    double *Dx, *Dy, *lmaxVx, *lmaxVy, *dVxdtau, *dVydtau, *dtauVx, *dtauVy, *dVx, *dVy, *betaVx, *betaVy, *cVx, *cVy, *alphaVx, *alphaVy, *Rx0, *Ry0;
    double *txx_v, *tyy_v, *toxx_v, *toyy_v, *lambda, *lambda_v, *dPpsi;
    const double *dT, *melt_fraction;
} jrx_dyrel2d_fields;
/* the keywords of _solve_DYREL! (solver.jl:55-66; defaults: viscosity_cutoff = (-Inf, Inf), viscosity_relaxation = 1e-2, λ_relaxation_DR = λ_relaxation_PH = 1,
 * iterMax = total_iterMax = 50e3, nout = 100, rel_drop = 1e-2, b_width = (4, 4, 0) [not read: one block], verbose_PH = verbose_DR = true, linear_viscosity = false)
 * and the scalars of the DYREL struct and of DYREL! (CFL = 0.99, ϵ = 1e-6, ϵ_vel = 1e-6, c_fact = 0.5, γfact = 20) */
typedef struct jrx_dyrel2d_params {
    double cutoff_lo, cutoff_hi, viscosity_relaxation, lambda_relaxation_DR, lambda_relaxation_PH;
    int64_t iterMax, total_iterMax, nout;
    double rel_drop;
    int32_t b_width[3], verbose_PH, verbose_DR, linear_viscosity;
    double CFL, eps, eps_vel, c_fact, gamma_fact;
} jrx_dyrel2d_params;
/* the named tuple _solve_DYREL! returns (solver.jl:292): err_evo_it / V / P / tot, caller buffers of cap entries (nchecks of them written), plus the counts */
typedef struct jrx_dyrel2d_result {
    int64_t iter, itPH, nchecks, cap;              /* inner iterations; Powell-Hestenes iterations; residual checks recorded; capacity of the buffers */
    double *err_evo_it, *err_evo_V, *err_evo_P, *err_evo_tot;
    double time_s;
} jrx_dyrel2d_result;
/* DYREL!(dyrel, stokes, rheology, phase_ratios, di, dt; CFL, γfact) -- constructors.jl:178-190: compute_bulk_viscosity_and_penalty!, the Gershgorin estimate, update_dτV_α_β! */
jrx_status jrx_dyrel2d_init(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                            const jrx_vep2d_params *p, const jrx_dyrel2d_params *dp);
/* _solve_DYREL! (solver.jl:44-294) with the epilogue :269-290 (P += ΔPψ, ∇V, vorticity, shear2center!, accumulate_tensor!, accumulate_vol!, τ_o = τ with xx_v, yy_v).
 * At entry P0 = P and ε_pl (xx, yy, xy_c), λ, λv are zeroed, as the reference does.  An inner iteration is three launches; the host reads the device sums once per
 * Powell-Hestenes iteration and once per nout inner iterations.  JRX_ERR_NAN for the reference's error("NaN detected ...") / error("Kaboom! ..."). */
jrx_status jrx_dyrel2d_solve(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rock_ratio2d *phi, const jrx_rheology *rh,
                             const jrx_vep2d_params *p, const jrx_dyrel2d_params *dp, jrx_dyrel2d_result *res);
/* the kernels alone, for parity tests.  compute_∇V_strain_rate_RP! (velocity_kernels.jl:154-240): ε.xx, ε.yy, ε.xy (do_strain_rate != 0) and R.RP; ∇V is not stored */
jrx_status jrx_dyrel2d_strain_rate_RP(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p, int32_t do_strain_rate);
/* compute_stress_viscosity_DRYEL! (stress_kernels.jl:100-307): τ (xx, yy, xy_c; xx_v, yy_v, xy), ε_pl, ε_vol_pl, τII, η_vep, λ, λv, ΔPψ, θc = γ_eff RP + ΔPψ in
 * d->P_num and, unless dp->linear_viscosity, η and ηv; of dp it reads viscosity_relaxation, the cutoff and linear_viscosity */
jrx_status jrx_dyrel2d_stress_viscosity(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh, const jrx_vep2d_params *p,
                                        const jrx_dyrel2d_params *dp, double lambda_relaxation);
/* compute_PH_residual_V! (velocity_kernels.jl:326-349): R.Rx, R.Ry from τ, P, ΔPψ, ρg */
jrx_status jrx_dyrel2d_PH_residual(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p);
/* compute_DR_residual_update_V! (velocity_kernels.jl:660-727): R / D, dVdτ <- α dVdτ + R, V += dVdτ β dτ; the ghosts are left to flow_bcs! */
jrx_status jrx_dyrel2d_DR_residual_update_V(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p);
/* Gershgorin_Stokes2D_SchurComplement! (Gershgorin.jl:1-155): Dx, Dy, λmaxVx, λmaxVy */
jrx_status jrx_dyrel2d_gershgorin(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh, const jrx_vep2d_params *p);
/* update_dτV_α_β! (Gershgorin.jl:216-247; from_lambda_max != 0) or update_α_β! (:171-198; dτV as it is, CFL not read) */
jrx_status jrx_dyrel2d_update_dtauV_alpha_beta(jrx_handle *h, const jrx_dyrel2d_fields *d, const jrx_vep2d_params *p, double CFL, int32_t from_lambda_max);
/* compute_bulk_viscosity_and_penalty! (constructors.jl:230-254): ηb, γ_eff; the mean of the finite η is reduced on the device */
jrx_status jrx_dyrel2d_bulk_viscosity_and_penalty(jrx_handle *h, const jrx_vep2d_fields *f, const jrx_dyrel2d_fields *d, const jrx_rheology *rh,
                                                  const jrx_vep2d_params *p, double gamma_fact);

/* ------------------------------------------------------------------ 3D DYREL (the 2D section above, one dimension up; it takes the 3D multiphase structs)
 * solve_DYREL!(stokes, ρg, dyrel, flow_bcs, phase_ratios, rheology, args, grid, dt, igg; kwargs...) on 3D grids.  The reference's 3D DYREL is half written.
 * Restated literally: the allocator DYREL(ni::NTuple{3}) (src/DYREL/constructors.jl:61-111), dyrel_fields(Val(3)), velocity_dofs, pressure_dof, compute_λminV!
 * (solver.jl:329-365), compute_∇V_strain_rate_RP! 3D (velocity_kernels.jl:242-322), compute_DR_residual_update_V! 3D (:729-828) and compute_PH_residual_V! 3D (:441-477)
 * apart from their shear differences (below), the N-dimensional update_α_β! / update_dτV_α_β! (Gershgorin.jl:171-310), compute_dV!, update_cV!,
 * compute_bulk_viscosity_and_penalty! (constructors.jl:230-254), the local law compute_local_stress / _compute_local_stress with its 6-component
 * empty_stress_solution (stress_kernels.jl:224-315) and the loop _solve_DYREL! (solver.jl:44-294).
 * No reference text -- the reference's compute_stress_viscosity_DRYEL! is 2D text and only Gershgorin_Stokes2D_SchurComplement! exists, so it cannot run a 3D solve:
 *   Stress kernel: compute_stress_viscosity_DRYEL! laid out as update_stresses_center_vertex_ps! 3D (src/stokes/StressKernels.jl:672-989).
 *     Centre: ε normals at the cell, each shear component the mean of the four surrounding edges of its family, τ_o = (xx, yy, zz, yz_c, xz_c, xy_c), η, P, λ,
 *     EII_pl and the centre ratios at the cell; the local law with 6 components; written: τ normals and the three centre shear copies, ε_pl normals, ε_vol_pl,
 *     τ.II, η_vep, λ, ΔPψ, θc = γ_eff RP + ΔPψ (P_num) and, unless linear_viscosity, η from the τII law (_update_τII_viscosity; its allzero·eps guard is taken
 *     over all six components and applied as compute_viscosity! 3D applies it, rheology/Viscosity.jl:481-492: τxx + ε, τyy - ε/2, τzz - ε/2), continuation ν, cutoff.
 *     Each edge family (yz, xz, xy) at its own extent, gathered as StressKernels.jl:705-733 and its siblings: η = harm_clamped_*(η); av_clamped_* of P, EII_pl,
 *     the ε normals and the τ_o normals; the edge's own shear of ε and τ_o; the other two shears through av_clamped_*_y / _z / _x; the ratios phase_ratios.yz / xz /
 *     xy; the local law with 6 components; kept: the edge's own shear stress, its plastic shear strain rate, its λv (three edge arrays).
 *     Departures from the 2D text: no vertex-normal stresses τ.xx_v / yy_v / zz_v (nor their τ_o twins) are read or written, so the epilogue's
 *     copy_stress_vertices!(..., Val(3)) is not performed; stokes.viscosity.ηv is neither read nor written; the τII refresh happens at the centres only, the
 *     edge viscosity being derived from η.  The edges of a call see the η of the previous call (the edge half runs before the centre half).
 *   Eigenvalue bound: Gershgorin_Stokes2D_SchurComplement! (Gershgorin.jl:21-155) one dimension up, over the operator these kernels apply.  Effective viscosity
 *     at every node 1 / (1/η + 1/(G dt)), η at an edge = harm_clamped_*(η), G from the node's own ratios.  For Vx at (i, j, k) of (nx-1, ny, nz), 1-based:
 *     E / W the centres [i+1,j,k] / [i,j,k], N / S the xy edges [i+1,j+1,k] / [i+1,j,k], T / B the xz edges [i+1,j,k+1] / [i+1,j,k];
 *       Dx  = (ηN+ηS)/dy² + (ηT+ηB)/dz² + (γE+γW + 4/3 (ηE+ηW))/dx²
 *       Cxx = |ηN|/dy² + |ηS|/dy² + |ηT|/dz² + |ηB|/dz² + |γE+4/3ηE|/dx² + |γW+4/3ηW|/dx² + |Dx|
 *       Cxy = (|γE-2/3ηE+ηN| + |γE-2/3ηE+ηS| + |γW-2/3ηW+ηN| + |γW-2/3ηW+ηS|)/(dx dy),   Cxz alike with T / B and dz;   λmaxVx = (Cxx + Cxy + Cxz)/Dx;
 *     Vy and Vz by cyclic permutation of the roles (Vy: yz edges across dz, xy edges across dx; Vz: xz edges across dx, yz edges across dy).
 *   Momentum residuals: the reference's 3D text takes the shear differences from _d_xi / _d_yi / _d_zi of MiniKernels.jl:53-55, which read A[i+1, j+1, k+1] --
 *     one plane past τxy, across two planes elsewhere.  Built instead: the index triples of the unmasked 3D velocity kernel (src/stokes/VelocityKernels.jl:215-238),
 *       Rx[i,j,k] = (τxx[i+1,j,k]-τxx[i,j,k])/dx + (τxy[i+1,j+1,k]-τxy[i+1,j,k])/dy + (τxz[i+1,j,k+1]-τxz[i+1,j,k])/dz - d_xa(P) - d_xa(θ) - av_x(ρgx),
 *     y and z alike; θ = ΔPψ (PH residual) or θc (DR residual).  These are the neighbours of the bound above.
 * Built: 3D, one block, uniform spacing, the table rheology of jrx_rheology (every visc_kind, ConstantElasticity, an optional DruckerPrager_regularised with the
 * softening laws, the density laws), free-slip / no-slip velocity boundary conditions, the plain pressure residual -∇V - (P - P0)/ηb + Q/dt, both values of
 * linear_viscosity.  Status JRX_ERR_ARG before anything is launched, with a text that names the cause, for: a handle with a communicator; a non-uniform Geometry
 * (inverse spacings that are not positive finite scalars: how a binding hands one over, this struct having no arrays for it); a RockRatio (phi non-NULL); an is_pl
 * other than 0 or 1; d->dT or d->melt_fraction non-NULL; periodic faces; a free_surface boundary condition (handed over as p->displacement_bcs = -1, this struct
 * having no member for it); fewer than 3 cells in a dimension; 2^31 or more entries in an array.
 * Of jrx_vep3d_params these entry points read nx, ny, nz, nxg, nyg, nzg, _dx, _dy, _dz, dt, free_slip, no_slip, periodic, displacement_bcs and T_ghosted.
 * jrx_dyrel2d_params and jrx_dyrel2d_result are reused: nothing in them is 2D-specific.  Counter "stat_dyrel_launches" counts these launches too.
 * jrx_dyrel3d_fields: the arrays of the DYREL struct (types.jl:24-59): γ_eff, ηb, P_num (ni); Dx, λmaxVx, dVxdτ, dτVx, dVx, βVx, cVx, αVx, Rx0 (nx-1, ny, nz), their y
 * members (nx, ny-1, nz) and z members (nx, ny, nz-1); then λ (ni), the three λv on the yz / xz / xy edges, ΔPψ (ni); then args.ΔT and args.melt_fraction (NULL). */
typedef struct jrx_dyrel3d_fields {
    double *gamma_eff, *etab, *P_num;
    double *Dx, *Dy, *Dz, *lmaxVx, *lmaxVy, *lmaxVz, *dVxdtau, *dVydtau, *dVzdtau, *dtauVx, *dtauVy, *dtauVz, *dVx, *dVy, *dVz;
    double *betaVx, *betaVy, *betaVz, *cVx, *cVy, *cVz, *alphaVx, *alphaVy, *alphaVz, *Rx0, *Ry0, *Rz0;
    double *lambda, *lambda_yz, *lambda_xz, *lambda_xy, *dPpsi;
    const double *dT, *melt_fraction;
} jrx_dyrel3d_fields;
/* DYREL!(dyrel, stokes, rheology, phase_ratios, di, dt; CFL, γfact) -- constructors.jl:178-190 with the 3D bound (no reference text) in the place of its 2D call */
jrx_status jrx_dyrel3d_init(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                            const jrx_vep3d_params *p, const jrx_dyrel2d_params *dp);
/* _solve_DYREL! (solver.jl:44-294) on a 3D grid.  At entry P0 = P and the centre members of ε_pl, λ and the three λv are zeroed; compute_viscosity!, compute_ρg!
 * (into ρg[3]), DYREL!; the Powell-Hestenes loop with rel_drop and err_min; norms over velocity_dofs(Val(3)) and pressure_dof, norm(D .* R) at the checks, errV00
 * from the first check; per check compute_λminV!, update_cV!, the 3D bound, update_dτV_α_β!; P += γ_eff RP after each velocity solve; epilogue P += ΔPψ,
 * compute_∇V!, compute_vorticity! 3D, shear2center! of ε / ε_pl / Δε, accumulate_tensor!, accumulate_vol!, τ_o = τ (normals, edge shears, centre shears).  An inner
 * iteration is four launches (strain rate + RP, stress edges, stress centres, update) plus flow_bcs!; the host reads the device sums once per Powell-Hestenes
 * iteration and once per nout inner iterations.  JRX_ERR_NAN for the reference's error("NaN detected ...") / error("Kaboom! ..."). */
jrx_status jrx_dyrel3d_solve(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rock_ratio3d *phi, const jrx_rheology *rh,
                             const jrx_vep3d_params *p, const jrx_dyrel2d_params *dp, jrx_dyrel2d_result *res);
/* the kernels alone, for parity tests.  compute_∇V_strain_rate_RP! 3D (velocity_kernels.jl:242-322): the six strain rates (do_strain_rate != 0) and R.RP */
jrx_status jrx_dyrel3d_strain_rate_RP(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p, int32_t do_strain_rate);
/* the 3D stress kernel (no reference text; the form stated above); of dp it reads viscosity_relaxation, the cutoff and linear_viscosity */
jrx_status jrx_dyrel3d_stress_viscosity(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p,
                                        const jrx_dyrel2d_params *dp, double lambda_relaxation);
/* compute_PH_residual_V! 3D (velocity_kernels.jl:441-477, shear differences as stated above): R.Rx, R.Ry, R.Rz from τ, P, ΔPψ, ρg */
jrx_status jrx_dyrel3d_PH_residual(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p);
/* compute_DR_residual_update_V! 3D (velocity_kernels.jl:729-828, shear differences as stated above): R / D, dVdτ <- α dVdτ + R, V += dVdτ β dτ; ghosts left to flow_bcs! */
jrx_status jrx_dyrel3d_DR_residual_update_V(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p);
/* the 3D eigenvalue bound (no reference text; the form stated above): Dx, Dy, Dz, λmaxVx, λmaxVy, λmaxVz */
jrx_status jrx_dyrel3d_gershgorin(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh, const jrx_vep3d_params *p);
/* update_dτV_α_β! (Gershgorin.jl:216-247, 290-310; from_lambda_max != 0) or update_α_β! (:171-198, 272-288; dτV as it is, CFL not read), three components */
jrx_status jrx_dyrel3d_update_dtauV_alpha_beta(jrx_handle *h, const jrx_dyrel3d_fields *d, const jrx_vep3d_params *p, double CFL, int32_t from_lambda_max);
/* compute_bulk_viscosity_and_penalty! (constructors.jl:230-254): ηb, γ_eff; the mean of the finite η is reduced on the device */
jrx_status jrx_dyrel3d_bulk_viscosity_and_penalty(jrx_handle *h, const jrx_vep3d_fields *f, const jrx_dyrel3d_fields *d, const jrx_rheology *rh,
                                                  const jrx_vep3d_params *p, double gamma_fact);

/* ------------------------------------------------------------------ per-step operators: pureshear_bc!, free_surface_bcs!, subgrid_characteristic_time!,
 * compute_melt_fraction!
 * What a time loop calls once per step around the solves.  Each is ONE launch, synchronous.  JRX_ERR_ARG (4) with a text naming the cause, nothing launched
 * and nothing written: a NULL pointer that is not optional, an extent < 1, a phase count outside 1..JRX_MAXPHASE, an array of 2^31 or more entries, a spacing
 * or dt that is not positive and finite, and what each operator lists.  Counter "stat_stepops_launches" (jrx_get_option): the kernels these six entry points
 * launched.
 *
 * pureshear_bc!(stokes, xci, xvi, εbg, backend) -- src/boundaryconditions/pure_shear.jl:1-33.  xv, yv[, zv]: device arrays of the nx+1, ny+1[, nz+1] vertex
 * coordinates (so a non-uniform Geometry works: no spacing enters); xci gives the reference only the extents, which are nx, ny[, nz] here.
 *   2D: Vx[:, 2:end-1] = εbg xv[i], Vy[2:end-1, :] = -εbg yv[j].
 *   3D: Vx[:, 2:end-1, 2:end-1] = εbg xv[i], Vy[2:end-1, :, 2:end-1] = εbg yv[j], Vz[2:end-1, 2:end-1, :] = -εbg zv[k].
 * The ghost rows, columns and planes are not touched.  The multiply is the only rounding.
 * NOT FOLLOWED in 3D: the reference's text iterates `y in xv` for Vy and `y in xc` for Vz (pure_shear.jl:23,28): Vy takes the x vertices, and the array
 * comprehensions fit size(Vy), size(Vz) only when nx == ny.  The form with yv is built; where nx == ny and xv == yv both give the same bits. */
jrx_status jrx_pureshear_bc2d(jrx_handle *h, double *Vx, double *Vy, const double *xv, const double *yv, double eps_bg, int64_t nx, int64_t ny);
jrx_status jrx_pureshear_bc3d(jrx_handle *h, double *Vx, double *Vy, double *Vz, const double *xv, const double *yv, const double *zv, double eps_bg,
                              int64_t nx, int64_t ny, int64_t nz);
/* free_surface_bcs!(stokes, flow_bcs, η, rheology, phase_ratios, dt, di...) -- src/boundaryconditions/free_surface.jl:1-99 (kernels FreeSurface_Vy! :38-68,
 * :70-99).  free_surface = flow_bcs.free_surface: 0 returns JRX_OK at once, nothing is launched.  phase_c: phase_ratios.center (nphase, ni...); of rh only
 * nphase and G are read: G = fn_ratio(get_shear_modulus, rheology, ratios of the top cell), the plain weighted sum (src/phases/phases.jl:6-15).
 *   2D, i = 1..nx, ν = 1e-2:  Vy[i+1, end] = ν (Vy[i+1, end-1] + 3/2 (P[i,end] / (2 η[i,end]) + (τ_o.yy[i,end] + P0[i,end]) / (2 G dt)
 *                                              + inv(3) (Vx[i+1, end-1] - Vx[i, end-1]) inv(dx)) dy) + (1 - ν) Vy[i+1, end]
 *   3D, (i, j) = (1..nx, 1..ny):  Vz[i+1, j+1, end] = Vz[i+1, j+1, end-1] + 3/2 (P / (2 η) + (τ_o.yy + P0) / (2 G dt)
 *                                              + inv(3) ((Vx[i+1, j+1, end-1] - Vx[i, j+1, end-1]) inv(dx) + (Vy[i+1, j+1, end-1] - Vy[i+1, j, end-1]) inv(dy))) dz
 *     with P, η, τ_o.yy, P0 at [i, j, end].
 * Grouping and operation order are the reference's, without fma.  Only Vy[2:end-1, end] (2D) / Vz[2:end-1, 2:end-1, end] (3D) is written.
 * KEPT QUIRK: the 3D form reads τ_o.yy, not τ_o.zz (free_surface.jl:28,76,91), as the reference does; tau_o_yy is that array.
 * Spacings: dx, dy[, dz] are used as the kernel uses them (inv(dx), ... dy).  2D: dx_i / dy_j, when not NULL, are the reference's spacing arrays _di_vx[1]
 * (nx entries, read at [i]) and _di_vy[2] (ny entries, read at [end]) -- members [0] and [1] of jrx_stokes2d_params.inv_spacing -- and replace the scalars;
 * the values are used as handed over (the reference's only, commented-out 2D call hands it the _di arrays: Stokes2D.jl:782).  3D: scalars only. */
jrx_status jrx_free_surface_bcs2d(jrx_handle *h, const double *Vx, double *Vy, const double *P, const double *P0, const double *tau_o_yy, const double *eta,
                                  const double *phase_c, const jrx_rheology *rh, double dt, double dx, double dy, const double *dx_i, const double *dy_j,
                                  int64_t nx, int64_t ny, int32_t free_surface);
jrx_status jrx_free_surface_bcs3d(jrx_handle *h, const double *Vx, const double *Vy, double *Vz, const double *P, const double *P0, const double *tau_o_yy,
                                  const double *eta, const double *phase_c, const jrx_rheology *rh, double dt, double dx, double dy, double dz, int64_t nx,
                                  int64_t ny, int64_t nz, int32_t free_surface);
/* subgrid_characteristic_time!(subgrid_arrays, particles, dt₀, phases, rheology, thermal, stokes[, di]) -- src/particles/subgrid_diffusion.jl:36-50 (the kernel;
 * its first two arguments are not read by it):  dt0[I] = ρCp / (2 K Σ_d inv(dx_d)^2), ρCp = compute_ρCp and K = compute_conductivity of the thermal phase table
 * averaged over the centre ratios of the cell (fn_ratio with args: a ratio of exactly 1 returns that phase alone, phases.jl:17-30), P = stokes.P[I],
 * T = thermal.T[I .+ 1].  T is the ghosted (ni .+ 2) array: I .+ 1 is the cell's OWN centre node in this layout (ghost layer at index 0), the same node
 * jrx_update_pt_thermal_arrays reads.  n = {nx, ny, nz} (nz = 1 in 2D), di = {dx, dy[, dz]}: uniform spacings.  Of ph, max_lxyz and Vpdtau are not read. */
jrx_status jrx_subgrid_characteristic_time(jrx_handle *h, double *dt0, const double *phase_c, const jrx_thermal_phases *ph, const double *T, const double *P,
                                           const int64_t n[3], int32_t ndim, const double di[3]);
/* compute_melt_fraction!(ϕ, [phase_ratios,] rheology, args) -- src/rheology/Melting.jl:10-35.  The melting laws of the phases as a table: kind 0 = no law
 * (ϕ = 0), kind 1 = MeltingParam_Caricchi: ϕ = 1 / (1 + exp((a - (T - c)) / b)), T in kelvin, defaults a = 800, b = 23, c = 273.15.  GeoParams is not part of
 * the reference tree; kind 1 is the one law whose form the reference's own test pins (test/test_rheology.jl:228-253: 0.95 < ϕ < 1 at 1373.15 K, ~3e-10 at
 * 573.15 K), so any other kind is refused by name ("melting") rather than written from memory. */
typedef struct jrx_melting {
    int32_t nphase;
    int32_t kind[JRX_MAXPHASE];
    double a[JRX_MAXPHASE], b[JRX_MAXPHASE], c[JRX_MAXPHASE];
} jrx_melting;
/* phase_c NULL: the single-material form, ϕ[I] = compute_meltfraction(phase 0, args[I]); otherwise fn_ratio over phase_ratios.center with the ratio == 1
 * shortcut (phases.jl:17-30).  args.T / args.P: T, P are arrays of the extent of ϕ read at the cell's own index (getindex_NamedTuple), or NULL, and then the
 * scalars T_scalar / P_scalar apply.  Neither law above reads P.  n = {nx, ny, nz} (nz = 1 in 2D). */
jrx_status jrx_compute_melt_fraction(jrx_handle *h, double *phi, const double *phase_c, const jrx_melting *m, const double *T, double T_scalar, const double *P,
                                     double P_scalar, const int64_t n[3], int32_t ndim);

/* ------------------------------------------------------------------ 2D marker-in-cell particles: advect, re-bucket, interpolate, phase ratios
 * The material of the reference's miniapps lives on JustPIC particles; per step they call advection!(particles, RungeKutta2(), @velocity(stokes), dt),
 * move_particles!(particles, particle_args), update_phase_ratios!(phase_ratios, particles, pPhases), with grid2particle! / particle2grid! around them
 * (miniapps/benchmarks/stokes2D/shear_heating/Shearheating2D.jl:69-82,221-232 gives the call shapes).  JustPIC's text is not in the reference tree, so nothing
 * is restated: what is built is defined HERE, to the rounding, and tests/_particles2d.py is the same text in NumPy.  Every operator is a GATHER with loops
 * bounded by max_xcell: nothing races, nothing depends on launch order, the device and the NumPy text leave the same bits.
 * Scope: 2D here (3D: the core chain, in the section after this one), uniform grid, one block (a handle with a communicator is refused), fp64.  NOT built: non-uniform grids, a marker chain,
 * force_injection!, clean_particles!, StressParticles (operators 6 - 9 below carry the stress through the reference's tuple methods instead),
 * grid2particle_flip!.
 *
 * Layout.  The grid has (nx, ny) cells of size (dx, dy), cell (i, j) = [x0 + i dx, x0 + (i+1) dx) x [y0 + j dy, y0 + (j+1) dy), 0-based.  Every cell owns a BUCKET
 * of max_xcell slots.  Every per-particle array -- px, py (coordinates), active (int32 mask: 1 = the slot holds a particle) and every particle field (pPhases, pT,
 * ...: fp64) -- is column-major of shape (nx, ny, max_xcell): entry (i, j, s) at i + nx (j + ny s).  The SLOT index is SLOWEST, so the threads of a wave (neighbouring
 * cells i) read neighbouring addresses in every slot loop: the accesses coalesce.  This is the opposite of the PhaseRatios layout (phase index fastest), which is
 * written, N contiguous doubles per thread.  A phase is stored as the double 1.0 ... N.  INVARIANT: an inactive slot holds 0 in every array (+0.0; active = 0); every
 * operator keeps it, and the bit-for-bit tests rely on it.  The bucket of a particle need not be its owner cell between an advection and the next move.
 * _dx = 1 / dx and _dy = 1 / dy are formed once on the host (checked: part->_dx == 1.0 / part->dx); nx ny max_xcell < 2^31 (32-bit offsets).
 *
 * Rounding: no fma (the library builds with -ffp-contract=off); every product and sum is rounded once, left to right as written.  (double)i is exact.
 * Safety: an index derived from a coordinate is range-checked ON THE DOUBLE before the conversion to int (v >= 0 && v < n), so a NaN or an infinite coordinate
 * is "outside", never a conversion.  No atomics except integer adds into the library's counter words; no loop on data.
 *
 * JRX_ERR_ARG (4) with a text naming the cause, nothing launched ("stat_particles_launches" unchanged) and nothing written: a NULL pointer, nx or ny < 1,
 * max_xcell < 1, 2^31 or more slots, x0 / y0 not finite, dx / dy not positive and finite, _dx / _dy not their inverses, dt not finite, nargs outside
 * 0 .. JRX_MAXPHASE, nphase outside 1 .. JRX_MAXPHASE, src and dst of a move sharing an array or differing in any scalar, a handle with a communicator. */
typedef struct jrx_particles2d {
    double *px, *py;
    int32_t *active;
    int64_t nx, ny;
    int32_t max_xcell;
    double x0, y0, dx, dy, _dx, _dy;
} jrx_particles2d;
/* 1. advection!(particles, RungeKutta2(), @velocity(stokes), dt) -- the midpoint rule (alpha = 0.5), per active slot, in place:
 *      (ux, uy) = V(x, y);  xm = x + (0.5 dt) ux,  ym = y + (0.5 dt) uy;  (wx, wy) = V(xm, ym);  x' = x + dt wx,  y' = y + dt wy.
 *    Vx is (nx+1, ny+2) with nodes at (x0 + i dx, y0 + (j - 0.5) dy), Vy is (nx+2, ny+1) with nodes at (x0 + (i - 0.5) dx, y0 + j dy): stokes.V with its ghost
 *    layers.  The node-grid origins (ox, oy) = (x0, y0 - 0.5 dy) and (x0 - 0.5 dx, y0) are formed once on the host.  A component A of extents (mx, my) at (x, y):
 *      sx = (x - ox) _dx;  fx = floor(sx);  i0 = fx >= 0 ? (fx < mx - 1 ? (int)fx : mx - 2) : 0;  tx = sx - (double)i0;   sy, j0, ty likewise with _dy, my
 *      A(x, y) = (1 - ty) ((1 - tx) A[i0, j0] + tx A[i0+1, j0]) + ty ((1 - tx) A[i0, j0+1] + tx A[i0+1, j0+1])
 *    A point outside the node box therefore EXTRAPOLATES linearly from the outermost pair of nodes (tx < 0 or tx > 1); nothing is clamped.  If sx or sy of any
 *    of the four evaluations is not finite (NaN or infinite coordinate), the particle is left exactly as it was. */
jrx_status jrx_particles2d_advect_rk2(jrx_handle *h, const jrx_particles2d *part, const double *Vx, const double *Vy, double dt);
/* 2. move_particles!(particles, particle_args) -- out of place: src is read, every array of dst and of args_dst is written in full.
 *    Owner of a particle: cx = (x - x0) _dx, fx = floor(cx); inside along x iff fx >= 0 && fx < nx (on the doubles), then ic = (int)fx; jc likewise.  A particle
 *    exactly on the upper boundary (or with a NaN coordinate) is outside.
 *    ONE thread per destination cell (i, j) fills its dst slots from 0 upward:
 *      first the active particles of src cell (i, j), in slot order, whose owner is (i, j);
 *      then, for dj = -1, 0, 1 (outermost) and di = -1, 0, 1, (0, 0) skipped, the active particles of src cell (i + di, j + dj) (where that cell exists), in
 *      slot order, whose owner is (i, j).
 *    A particle that finds all max_xcell slots taken is dropped and counted in n_overflow.  The remaining dst slots are zeroed (coordinates, mask, args).
 *    Over its own src cell the same thread counts the active particles (n_active_before), those whose owner is outside the grid (n_outside) and those inside the
 *    grid whose owner is more than one cell away along x or y (n_far): nobody gathers these, they are lost.  n_active_after counts the filled dst slots.
 *    args_src / args_dst: host arrays of nargs device pointers (particle fields and their twins; may be NULL when nargs = 0).
 *    counts = {n_active_before, n_active_after, n_outside, n_far, n_overflow}; n_active_before = n_active_after + n_outside + n_far + n_overflow.
 *    One launch plus one read of the five counter words. */
jrx_status jrx_particles2d_move(jrx_handle *h, const jrx_particles2d *src, const jrx_particles2d *dst, const double *const *args_src, double *const *args_dst,
                                int32_t nargs, int64_t counts[5]);
/* 3. grid2particle!(pF, xvi, F, particles): F is a vertex field (nx+1, ny+1).  Per active slot (i, j, s), bilinear over the four vertices of the slot's BUCKET
 *    cell (i, j) -- not of the owner recomputed from the coordinate:
 *      tx = (x - (x0 + (double)i dx)) _dx,  ty = (y - (y0 + (double)j dy)) _dy,  pF = (1 - ty) ((1 - tx) F[i, j] + tx F[i+1, j]) + ty ((1 - tx) F[i, j+1] + tx F[i+1, j+1]).
 *    An inactive slot of pF is set to 0. */
jrx_status jrx_particles2d_grid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles2d *part);
/* 4. particle2grid!(F, pF, xvi, particles): one thread per vertex (i, j), xv = x0 + (double)i dx, yv = y0 + (double)j dy, reads its up to four cells at offsets
 *    {-1, 0}: the first dimension's offset outermost, -1 before 0 (the order of jrx_update_phase_ratios2d), cells outside the grid skipped, slots in order:
 *      w = (1 - fabs(x - xv) _dx) (1 - fabs(y - yv) _dy);  num += w pF;  den += w;     F[i, j] = num / den;  where den == 0, F[i, j] is left as it was. */
jrx_status jrx_particles2d_particle2grid(jrx_handle *h, double *F, const double *pF, const jrx_particles2d *part);
/* 5. update_phase_ratios!(phase_ratios, particles, pPhases): center (nphase, nx, ny), vertex (nphase, nx+1, ny+1), Vx (nphase, nx+1, ny), Vy (nphase, nx, ny+1),
 *    phase index fastest.  One launch, one thread per node (i, j) of the (nx+1, ny+1) box writes every member it owns.  With xv, yv as in (4) and the centres
 *    xc = x0 + ((double)i + 0.5) dx, yc = y0 + ((double)j + 0.5) dy:
 *      center[i, j]  (i < nx, j < ny): cell (i, j), weights to (xc, yc);         vertex[i, j]: the four cells of (4) in that order, weights to (xv, yv);
 *      Vx[i, j]  (j < ny): cells (i-1, j), (i, j), weights to (xv, yc);           Vy[i, j]  (i < nx): cells (i, j-1), (i, j), weights to (xc, yv).
 *    Weights as in (4) with the node's coordinates.  Per active slot: p = pPhases; skipped unless p >= 1 && p < nphase + 1; k = (int)p; w_k += w; W += w, slots
 *    in order.  ratio_k = w_k / W.  Where W == 0 the member is left unchanged and counted: *n_empty = the number of (node, member) pairs with W == 0. */
jrx_status jrx_particles2d_phase_ratios(jrx_handle *h, double *center, double *vertex, double *Vx, double *Vy, const double *pPhases, int32_t nphase,
                                        const jrx_particles2d *part, int64_t *n_empty);
/* Operators 6 - 9 carry the elastic stress on the particles: rotate_stress!(pτxx, pτyy, pτxy, pω, stokes, particles, dt), stress2grid!(stokes, pτxx, pτyy, pτxy,
 * particles) and rotate_stress_particles!((τ...), (ω,), particles, dt) -- the tuple methods of src/stress_rotation/stress_rotation_particles.jl:92-99,224-235,
 * 264-276 (StressParticles, the wrapper type of :205-222, is not built) -- and the two JustPIC operators they call, centroid2particle! / particle2centroid!,
 * which every thermal miniapp needs too (centroid2particle!(pT, T_buffer, particles)).  Layout, rounding, safety and refusals as above; further refusals: nx < 2
 * or ny < 2 where operator 6 is involved, an unknown method, an output that overlaps an input, another output or the particles' own arrays.
 * 6. centroid2particle!(pF, F, particles): F is a centre field (nx, ny), nodes at (x0 + (i + 0.5) dx, y0 + (j + 0.5) dy).  Per active slot pF = A(x, y), A the
 *    interpolant of (1) with extents (nx, ny) and node-grid origin (x0 + 0.5 dx, y0 + 0.5 dy), formed once on the host: the pair is found from the COORDINATE (not
 *    from the bucket), and a particle in the outer half cells extrapolates linearly from the outermost pair of centres.  A slot whose scaled coordinate is not
 *    finite is left as it was; an inactive slot is set to 0.  Needs nx >= 2 && ny >= 2. */
jrx_status jrx_particles2d_centroid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles2d *part);
/* 7. particle2centroid!(F, pF, particles): one thread per cell (i, j) walks its own bucket in slot order; xc = x0 + ((double)i + 0.5) dx, yc likewise;
 *      w = (1 - fabs(x - xc) _dx) (1 - fabs(y - yc) _dy);  num += w pF;  den += w;     F[i, j] = num / den;  where den == 0, F[i, j] is left as it was
 *    (the `center` rule of (5)). */
jrx_status jrx_particles2d_particle2centroid(jrx_handle *h, double *F, const double *pF, const jrx_particles2d *part);
/* 8. rotate_stress_particles!((pτxx, pτyy, pτxy), (pω,), particles, dt; method): per active slot, in place, θ = dt pω, then JRX_ROTATE_MATRIX or
 *    JRX_ROTATE_JAUMANN exactly as jrx_rotate_stress2d defines them per point (one device function serves both).  The reference's particle Jaumann kernel
 *    (:151-167) has the sign defect listed with jrx_rotate_stress2d and is not followed; its `method` keyword does not select an algorithm, here it does.
 *    An inactive slot is not touched (it holds 0).  ptau = {pτxx, pτyy, pτxy}: a HOST array of DEVICE pointers. */
jrx_status jrx_particles2d_rotate(jrx_handle *h, double *const ptau[3], const double *pomega, const jrx_particles2d *part, double dt, int32_t method);
/* 9. The two calls of a time step.  rotate_stress!: (6) of tau_xx into pτxx, (6) of tau_yy into pτyy, (3) of tau_xy into pτxy, (3) of omega_xy into pω, then (8).
 *    stress2grid!: tau_o = {xx, yy, xy_c, xy, xx_v, yy_v} (the member order of jrx_rotate_stress2d; all six required); xx, yy, xy_c from pτxx, pτyy, pτxy by (7),
 *    xx_v, yy_v, xy from pτxx, pτyy, pτxy by (4).  Each is defined as that chain and built as ONE launch that leaves the chain's bits in every output, corner cases
 *    included (inactive slots; a non-finite coordinate keeps pτxx, pτyy and sends what (3) makes of it through (8)): a thread per cell reads active, x, y of a
 *    slot once and writes the four particle fields; a thread per node of the (nx+1, ny+1) box loads each particle of its up to four cells once, in the cell and
 *    slot order of (4), the own cell also feeding the centre it owns (i < nx && j < ny) in the order of (7).  Tuning key "particles_stress_fused"
 *    (include/jrx_tuning.h) = 0 runs the chains: 5 and 6 launches. */
jrx_status jrx_particles2d_rotate_stress(jrx_handle *h, double *const ptau[3], double *pomega, const double *tau_xx, const double *tau_yy, const double *tau_xy,
                                         const double *omega_xy, const jrx_particles2d *part, double dt, int32_t method);
jrx_status jrx_particles2d_stress2grid(jrx_handle *h, double *const tau_o[6], const double *const ptau[3], const jrx_particles2d *part);
/* Operators 10 and 11 carry the TEMPERATURE on the particles: subgrid_diffusion_centroid!(pT, T_buffer, thermal.ΔT, subgrid_arrays, particles, dt) and
 * subgrid_diffusion!(...) with subgrid_arrays of loc = :vertex -- JustPIC's, as every thermo-mechanical miniapp of the reference calls them behind
 * heatdiffusion_PT! (miniapps/subduction/2D/Subduction2D.jl:221-243, test/test_Blankenbach.jl:225, test/test_thermalstresses.jl:420, docs/src/man/advection.md:42-53),
 * the one consumer of jrx_subgrid_characteristic_time (whose dt₀ the caller brings to the particles with (6)).  The scheme is Gerya & Yuen's subgrid diffusion;
 * tests/_particles2d_subgrid.py is this text in NumPy.  Layout, rounding, the +0.0 invariant, safety and refusals as above.
 * 10. subgrid_diffusion_centroid!.  pT (read and written), pT0, pdT (= pΔT) and pdt0 (= dt₀, read only) are particle fields; T_grid (the grid temperature BEFORE
 *    the diffusion solve, the miniapps' T_buffer) and dT_subgrid (= ΔT_subgrid, written) are centre fields (nx, ny); dT_grid, the grid change of the solve, read
 *    only, is (nx, ny) with dT_extent = JRX_SUBGRID_DT_NODES, or thermal.ΔT itself, (nx+2, ny+2) read at the cell's own node [i+1, j+1], with
 *    JRX_SUBGRID_DT_GHOSTED (the convention of args.ΔT of the multiphase drivers; the ghost entries are not read).  d in [0, 1], dt >= 0.  The operator is this CHAIN:
 *      1. pT0 = pT, every slot.
 *      2. pT = (6) of T_grid (so a slot whose scaled coordinate is not finite keeps its value, which is pT0).
 *      3. per active slot, a = pdt0:  m = a > 1e-9 ? a : 1e-9 (a NaN gives 1e-9);  x = ((-d) dt) / m, the product formed once on the host;  f = 1 - exp(x);
 *         δ = (pT - pT0) f;  pT0 = pT0 + δ;  pdT = δ.  An inactive slot of pdT is set to 0.
 *      4. dT_subgrid = +0.0 everywhere, then (7) of pdT into it (a cell with den == 0 keeps the 0).
 *      5. dT_subgrid[i, j] = dT_grid[i, j] - dT_subgrid[i, j].
 *      6. pdT = (6) of dT_subgrid (a slot whose scaled coordinate is not finite keeps δ).
 *      7. per active slot pT = pT0 + pdT; an inactive slot of pT is set to 0.
 *    Afterwards pT0 holds pT0 + δ, pdT the interpolated remainder, dT_subgrid the remainder.  exp is the device's: against NumPy d = 0 is bit for bit (exp(-0) = 1),
 *    d > 0 differs by that one function.  Needs nx >= 2 && ny >= 2.
 *    Built as TWO launches that leave the chain's bits in pT, pT0, pdT and dT_subgrid: a thread per cell walks its bucket once, does 1 - 3 per slot with the
 *    interpolated temperature in a register, accumulates num and den of (7) in slot order -- (7) reads only the cell's own bucket -- and writes
 *    dT_grid - num / den; a second launch does 6 and 7 (it reads the neighbours' remainders).
 * 11. subgrid_diffusion! with loc = :vertex: the same seven steps with (3) in place of (6) and (4) in place of (7) -- so a non-finite coordinate gives NaN, as (3)
 *    does -- and T_grid, dT_grid, dT_subgrid vertex fields (nx+1, ny+1); JRX_SUBGRID_DT_GHOSTED: (nx+3, ny+3) read at [i+1, j+1].  THREE launches: per cell
 *    (1 - 3), per vertex (the four-cell gather of (4) and the subtraction), per cell (6, 7).
 *    Tuning key "particles_subgrid_fused" (include/jrx_tuning.h) = 0 runs the chains: 7 launches each (steps 1, 2, 3, the launch of 4, 5, 6, 7; the fill of 4 is
 *    a memset).  Further refusals: d outside [0, 1] or not finite, dt negative or not finite, another dT_extent. */
#define JRX_SUBGRID_DT_NODES 0
#define JRX_SUBGRID_DT_GHOSTED 1
jrx_status jrx_particles2d_subgrid_diffusion_centroid(jrx_handle *h, double *pT, const double *T_grid, const double *dT_grid, int32_t dT_extent, double *pT0,
                                                      double *pdT, const double *pdt0, double *dT_subgrid, const jrx_particles2d *part, double d, double dt);
jrx_status jrx_particles2d_subgrid_diffusion_vertex(jrx_handle *h, double *pT, const double *T_grid, const double *dT_grid, int32_t dT_extent, double *pT0, double *pdT,
                                                    const double *pdt0, double *dT_subgrid, const jrx_particles2d *part, double d, double dt);
/* 12. inject_particles_phase!(particles, pPhases, args, fields) -- every particle miniapp of the reference calls it right after move_particles!, in every time step
 *    (miniapps/subduction/2D/Subduction2D.jl:246-263 with five vertex fields, SinkingBlock2D.jl:182 with (), (), test/test_shearheating2D.jl:215 with (pT,),
 *    (T_buffer,)): a cell left with fewer than min_xcell particles is refilled.  JustPIC places the new particles at random; HERE the placement is deterministic
 *    -- the empty sites of the sub-cell lattice of init_particles -- so that tests/_particles2d_inject.py restates it and the device leaves the same bits.
 *    Layout, rounding (no fma), safety and the +0.0 invariant as above.  GATHER form: ONE launch, one thread per cell (i, j), plus one read of the counter words.
 *    Donor set: the slots with active != 0 AT ENTRY (the mask holds 0 or 1).  No such slot is written, in any array: a thread reads only what nobody writes, and
 *    there are no float atomics.  The MASK is therefore written OUT OF PLACE: active_out[i, j, s] is written for every slot, a copy of part->active with 1 in the
 *    slots this call fills; px, py, pPhases and args[k] are written in place, and only in slots inactive at entry.  The caller then makes active_out the mask.
 *    nsx, nsy: the sub-cell lattice (init_particles: nsx the largest divisor of nxcell not above its square root, nsy = nxcell / nsx); hx = dx / nsx and
 *    hy = dy / nsy are formed once on the host.  For cell (i, j):
 *      1. n = the number of active slots of the cell's own bucket.  If n >= min_xcell the mask is copied and nothing else happens.
 *      2. Otherwise the cell is DEFICIENT (n_deficient).  xc = x0 + (double)i dx, yc = y0 + (double)j dy.
 *      3. Occupancy of the nsx x nsy lattice over the active slots of the own bucket, in slot order: a = floor(((x - xc) _dx) (double)nsx), b likewise with y, yc,
 *         _dy, nsy; site q = a + nsx b is occupied iff a >= 0 && a < nsx && b >= 0 && b < nsy, tested on the doubles.  A NaN or infinite coordinate, or a particle
 *         not yet moved into its owner cell, occupies no site; it still counts in n.  The occupancy is one 64-bit word: nsx nsy <= 64.
 *      4. For q = 0 .. nsx nsy - 1 in order (a = q mod nsx, b = q div nsx), while n < min_xcell, occupied sites skipped: the new point is
 *         x = xc + ((double)a + 0.5) hx, y = yc + ((double)b + 0.5) hy -- the bits init_particles gives without rng.
 *      5. Its donor: the cell's own bucket first, then the eight neighbours in the order of (2) (dj = -1, 0, 1 outermost, di = -1, 0, 1, cells outside the grid
 *         skipped), slots in order: ex = xd - x; ey = yd - y; d2 = ex ex + ey ey; a candidate wins iff d2 < best, best starting at +infinity.  The first of
 *         equals stays; a NaN or infinite d2 never wins.
 *      6. No donor: the cell is counted ONCE in n_no_donor and left as it is from there on (it heals in a later step, once its neighbours are filled).
 *      7. Otherwise the new particle goes into the lowest slot of the bucket that was inactive at entry and has not been filled in this call: coordinates (x, y),
 *         1 in active_out, pPhases = the donor's, and args[k] by field_loc[k]: JRX_INJECT_VERTEX -- fields[k] is (nx+1, ny+1), the expression of (3) at (x, y)
 *         over the vertices of cell (i, j); JRX_INJECT_CENTRE -- fields[k] is (nx, ny), A(x, y) of (6) (not written if a scaled coordinate is not finite);
 *         JRX_INJECT_DONOR -- fields[k] is not read (may be NULL), args[k] of the donor's slot.  n++, n_injected++.
 *      8. There are always enough sites: occupied sites <= n < min_xcell <= nsx nsy.
 *    A particle field that is not listed keeps +0.0 in the new slot.  args, fields: HOST arrays of nargs DEVICE pointers, field_loc a host array (all three may be
 *    NULL when nargs = 0).  counts = {n_active_before, n_active_after, n_deficient, n_injected, n_no_donor}; n_active_after = n_active_before + n_injected.
 *    Further refusals: min_xcell < 1, > max_xcell or > nsx nsy; nsx or nsy < 1, nsx nsy > 64; an unknown field_loc; JRX_INJECT_CENTRE with nx < 2 or ny < 2;
 *    active_out overlapping the mask; pPhases, any args[k], active_out and the particles' arrays not pairwise disjoint; a fields[k] that is read overlapping
 *    anything written. */
#define JRX_INJECT_VERTEX 0   /* fields[k] is (nx+1, ny+1): operator 3's form at the new point        */
#define JRX_INJECT_CENTRE 1   /* fields[k] is (nx, ny): operator 6's interpolant A(x, y); nx, ny >= 2 */
#define JRX_INJECT_DONOR  2   /* fields[k] is not read: the value of args[k] in the donor's slot      */
jrx_status jrx_particles2d_inject(jrx_handle *h, const jrx_particles2d *part, int32_t *active_out, double *pPhases, double *const *args, const double *const *fields,
                                  const int32_t *field_loc, int32_t nargs, int32_t min_xcell, int32_t nsx, int32_t nsy, int64_t counts[5]);

/* ------------------------------------------------------------------ 3D marker-in-cell particles: advect, re-bucket, interpolate, phase ratios
 * The core chain of the reference's 3D miniapps (miniapps/benchmarks/stokes3D/shear_heating/Shearheating3D.jl:63-78,224-233: init_particles, init_cell_arrays,
 * advection!, move_particles!, particle2centroid!, update_phase_ratios!) on the layout and under the rules of the 2D section above, which this section EXTENDS:
 * operators 1 - 7 there, with a third index.  tests/_particles3d.py is this text in NumPy.  Every operator is a gather with loops bounded by max_xcell; no atomics
 * except integer adds into the counter words; no fma, every product and sum rounded once, left to right; an index derived from a coordinate is range-checked on
 * the double before the conversion; an inactive slot holds +0.0 / 0 in every array.
 * Scope: 3D, uniform grid, one block, fp64.  NOT built in 3D: inject_particles_phase!, the stress operators (8, 9), subgrid diffusion (10, 11), non-uniform
 * grids, decomposed grids (a handle with a communicator is refused), marker chains, StressParticles.  Without injection a flow that crosses the boundary loses
 * material there; n_outside reports it.
 *
 * Layout.  (nx, ny, nz) cells of size (dx, dy, dz); every per-particle array is (nx, ny, nz, max_xcell) column-major, the SLOT index slowest: entry (i, j, k, s) at
 * i + nx (j + ny (k + nz s)).  nx ny nz max_xcell < 2^31 and (nx+2)(ny+2)(nz+2) < 2^31 (32-bit offsets).  _dx, _dy, _dz are formed once on the host (checked).
 * Grid fields are column-major; phase-ratio members have the phase index fastest.
 *
 * JRX_ERR_ARG with a text naming the cause, nothing launched ("stat_particles_launches" unchanged) and nothing written: as in 2D -- a NULL pointer, an extent
 * < 1, max_xcell < 1, 2^31 or more slots, an origin that is not finite, a spacing that is not positive and finite, _dx / _dy / _dz not the inverses, dt not
 * finite, nargs outside 0 .. JRX_MAXPHASE, nphase outside 1 .. JRX_MAXPHASE, src and dst of a move sharing an array or differing in a scalar, an output that
 * overlaps an input, another output or the particles' own arrays, an extent < 2 for operator 6, a handle with a communicator. */
typedef struct jrx_particles3d {
    double *px, *py, *pz;
    int32_t *active;
    int64_t nx, ny, nz;
    int32_t max_xcell;
    double x0, y0, z0, dx, dy, dz, _dx, _dy, _dz;
} jrx_particles3d;
/* 1. advection!(particles, RungeKutta2(), @velocity(stokes), dt) -- the midpoint rule of 2D operator 1 with three components:
 *      (ux, uy, uz) = V(x, y, z);  xm = x + (0.5 dt) ux, ym, zm likewise;  (wx, wy, wz) = V(xm, ym, zm);  x' = x + dt wx,  y' = y + dt wy,  z' = z + dt wz.
 *    Vx is (nx+1, ny+2, nz+2) with nodes at (x0 + i dx, y0 + (j - 0.5) dy, z0 + (k - 0.5) dz), Vy is (nx+2, ny+1, nz+2), Vz is (nx+2, ny+2, nz+1), likewise:
 *    stokes.V with its ghost layers; the origins x0 - 0.5 dx, ... are formed once on the host.  Per axis s, i0, t exactly as in 2D (so a point outside the node
 *    box extrapolates).  With B(m) the 2D bilinear expression on the plane k0 + m,
 *      A(x, y, z) = (1 - tz) B(0) + tz B(1).
 *    If any scaled coordinate of any of the six evaluations is not finite, the particle is left exactly as it was. */
jrx_status jrx_particles3d_advect_rk2(jrx_handle *h, const jrx_particles3d *part, const double *Vx, const double *Vy, const double *Vz, double dt);
/* 2. move_particles!(particles, particle_args) -- out of place.  Owner per axis as in 2D (fx = floor((x - x0) _dx), inside iff fx >= 0 && fx < nx on the double).
 *    ONE thread per destination cell (i, j, k) fills its dst slots from 0 upward: first the active particles of src cell (i, j, k), in slot order, whose owner
 *    is (i, j, k); then, for dk = -1, 0, 1 (outermost), dj = -1, 0, 1, di = -1, 0, 1 (innermost), (0, 0, 0) skipped, the active particles of src cell
 *    (i + di, j + dj, k + dk) (where that cell exists), in slot order, whose owner is (i, j, k).  A particle that finds the bucket full is counted in n_overflow;
 *    the remaining dst slots are zeroed.  Over its own cell a thread counts n_active_before, n_outside and n_far (the owner is inside the grid and more than one
 *    cell away along any axis).  counts and their sum rule as in 2D.
 *    work: NULL, or a device buffer of nx ny nz max_xcell BYTES owned by the caller, disjoint from everything else.  NULL (or tuning key
 *    "particles3d_move_codes" = 0): the direct form, one launch -- a destination cell computes the owner of every particle of its 27 cells from the three
 *    coordinates.  With work: two launches -- a pre-pass, a thread per source cell, stores each slot's owner in one byte ((dk+1) 9 + (dj+1) 3 + (di+1) for a
 *    neighbour offset, 255 inactive, 254 outside, 253 far) and takes n_active_before, n_outside, n_far; the gather reads the bytes of its 27 cells and loads
 *    coordinates and fields only of the slots it takes.  Both forms leave identical bits in every output and counter. */
jrx_status jrx_particles3d_move(jrx_handle *h, const jrx_particles3d *src, const jrx_particles3d *dst, const double *const *args_src, double *const *args_dst,
                                int32_t nargs, uint8_t *work, int64_t counts[5]);
/* 3. grid2particle!(pF, xvi, F, particles): F is a vertex field (nx+1, ny+1, nz+1).  Per active slot (i, j, k, s), trilinear over the eight vertices of the slot's
 *    BUCKET cell: tx = (x - (x0 + (double)i dx)) _dx, ty, tz likewise, combined as in (1).  An inactive slot of pF is set to 0. */
jrx_status jrx_particles3d_grid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles3d *part);
/* 4. particle2grid!(F, pF, xvi, particles): one thread per vertex (i, j, k) reads its up to eight cells at offsets {-1, 0}: the first dimension's offset
 *    outermost, the third innermost, -1 before 0 (the order of jrx_update_phase_ratios3d), cells outside the grid skipped, slots in order:
 *      w = (1 - fabs(x - xv) _dx) (1 - fabs(y - yv) _dy) (1 - fabs(z - zv) _dz);  num += w pF;  den += w;     F = num / den;  where den == 0, F is left as it was. */
jrx_status jrx_particles3d_particle2grid(jrx_handle *h, double *F, const double *pF, const jrx_particles3d *part);
/* 5. update_phase_ratios!(phase_ratios, particles, pPhases): members[8] = center, vertex, Vx, Vy, Vz, yz, xz, xy (a HOST array of device pointers), each
 *    (nphase, nx + sx, ny + sy, nz + sz) with the stagger (sx, sy, sz) = (0,0,0), (1,1,1), (1,0,0), (0,1,0), (0,0,1), (0,1,1), (1,0,1), (1,1,0).  A member exists at
 *    node (i, j, k) when i < nx + sx, j < ny + sy, k < nz + sz.  It gathers the cells at offsets {-1, 0} along its staggered axes and {0} along the others, in the
 *    nesting order of (4); the weight of (4) goes to the vertex coordinate x0 + (double)i dx along a staggered axis and to the centre coordinate
 *    x0 + ((double)i + 0.5) dx along the others.  Phase acceptance, ratio_k = w_k / W and the W == 0 rule (member left unchanged, counted in *n_empty) as in 2D.
 *    One launch, or two launches of four members each at nphase = JRX_MAXPHASE (the same bits; tuning key "particles3d_ratios_split"). */
jrx_status jrx_particles3d_phase_ratios(jrx_handle *h, double *const members[8], const double *pPhases, int32_t nphase, const jrx_particles3d *part,
                                        int64_t *n_empty);
/* 6. centroid2particle!(pF, F, particles): F is a centre field (nx, ny, nz).  Per active slot pF = A(x, y, z), A the interpolant of (1) with extents (nx, ny, nz)
 *    and node-grid origin (x0 + 0.5 dx, y0 + 0.5 dy, z0 + 0.5 dz): the pair is found from the COORDINATE, the outer half cells extrapolate.  A slot whose scaled
 *    coordinate is not finite is left as it was; an inactive slot is set to 0.  Needs every extent >= 2. */
jrx_status jrx_particles3d_centroid2particle(jrx_handle *h, double *pF, const double *F, const jrx_particles3d *part);
/* 7. particle2centroid!(F, pF, particles): one thread per cell walks its own bucket in slot order, weights of (4) to the centre; an empty cell keeps its value. */
jrx_status jrx_particles3d_particle2centroid(jrx_handle *h, double *F, const double *pF, const jrx_particles3d *part);

#ifdef __cplusplus
}
#endif
#endif /* JRX_H */
