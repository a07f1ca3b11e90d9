/*
 * fv3_mi355x.h -- C ABI of the MI355X-native FV3 acoustic dynamics.
 *
 * Drop-in boundary for the hot path pace reaches through
 *   Driver._critical_path_step_all -> DynamicalCore.step_dynamics -> AcousticDynamics
 *   [REF driver/pace/driver/driver.py:494-504, 641]
 * One entry point per operator object the reference constructs through
 * StencilFactory / QuantityFactory [REF driver/pace/driver/driver.py:744-765;
 * examples/notebooks/functions.py:877-891, 935-951].  pyFV3 itself is an
 * un-vendored submodule, so each entry point cites the reference evidence for
 * the operator it replaces (class name / checkpoint variables / config field).
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / numpy types cross this ABI.
 *  - every 3-D field of a context shares ONE layout: [n_sub][nk_alloc][nj_alloc][ni_alloc],
 *    i fastest (stride 1).  Logical index order is the reference's (i, j, k)
 *    [REF tests/main/fv3core/test_init_from_geos.py:94-113]; fields are padded to the
 *    interface shape (nx+2h+1, ny+2h+1, nz+1) like NDSL storages.
 *  - n_sub sub-domains (ranks of the reference) are co-resident in one context and
 *    processed by the same launches ("6 tiles on 1 GPU", BASELINE cfg-1).
 *  - all calls are asynchronous on the given hipStream_t (passed as void*); the
 *    library never allocates at call time (scratch is owned by the context), mirroring
 *    the reference invariants [REF tests/main/fv3core/test_dycore_call.py:193-211].
 *  - return 0 on success, negative fv3_status otherwise; fv3_last_error() has the text.
 *    Nothing throws across the boundary.
 */
#ifndef FV3_MI355X_H
#define FV3_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV3_MAX_SUB 32
#define FV3_ABI_VERSION 2

typedef enum {
  FV3_OK = 0,
  FV3_ERR_ARG = -1,         /* bad pointer / shape / stride / dtype ("validate_args") */
  FV3_ERR_HIP = -2,         /* a HIP runtime call failed */
  FV3_ERR_UNSUPPORTED = -3, /* configuration outside the specialised set */
  FV3_ERR_NOMEM = -4
} fv3_status;

typedef enum { FV3_F64 = 0, FV3_F32 = 1 } fv3_dtype;

/* edge flag bits per sub-domain == GridIndexing.{west,east,south,north}_edge
 * [REF tests/main/fv3core/test_grid.py:56-101] */
#define FV3_EDGE_W 1
#define FV3_EDGE_E 2
#define FV3_EDGE_S 4
#define FV3_EDGE_N 8

typedef struct fv3_ctx fv3_ctx;

/* A borrowed view of one Quantity's storage (all sub-domains). */
typedef struct {
  void *ptr;
  int64_t shape[3];   /* logical (i, j, k) extents of the allocation */
  int64_t stride[3];  /* element strides for (i, j, k); stride[0] must be 1 */
  int64_t sub_stride; /* elements between consecutive sub-domains */
  int32_t n_sub;
  int32_t dtype;      /* fv3_dtype */
} fv3_field;

/* GridIndexing / sizer [REF driver/pace/driver/driver.py:744-765] */
typedef struct {
  int32_t nx, ny, nz, n_halo, n_sub;
  int32_t edge_flags[FV3_MAX_SUB];
} fv3_gridspec;

/* GridData + DampingCoefficients, device pointers, 2-D fields laid out
 * [n_sub][nj_alloc][ni_alloc]  [REF tests/mpi_54rank/test_grid_init.py:33-120] */
typedef struct {
  const void *dx, *dy, *dxa, *dya, *dxc, *dyc;
  const void *rdx, *rdy, *rdxa, *rdya, *rdxc, *rdyc;
  const void *area, *rarea, *area_c, *rarea_c;
  const void *cosa, *sina, *rsina, *cosa_u, *cosa_v, *cosa_s;
  const void *sina_u, *sina_v, *rsin_u, *rsin_v, *rsin2;
  const void *sin_sg1, *sin_sg2, *sin_sg3, *sin_sg4;
  const void *cos_sg1, *cos_sg2, *cos_sg3, *cos_sg4;
  const void *fC, *f0;
  const void *del6_u, *del6_v, *divg_u, *divg_v;
  const void *edge_w, *edge_e; /* [n_sub][nj_alloc] */
  const void *edge_s, *edge_n; /* [n_sub][ni_alloc] */
  /* host arrays (copied at create) */
  const double *corner_extrap; /* [n_sub][4][3] a2b_ord4 cube-corner factors */
  const double *ak, *bk;       /* [nz+1] */
  double da_min, da_min_c;
  const void *sin_sg5; /* (ABI 2) sine of the grid angle at the cell centre: tracer_2d_1l's Courant bound; may be NULL if unused */
} fv3_griddata;

/* dycore_config fields the acoustic path reads
 * [REF driver/examples/configs/baroclinic_c12.yaml:43-93] */
typedef struct {
  int32_t n_split, k_split;
  int32_t hord_dp, hord_mt, hord_tm, hord_vt;
  int32_t nord, n_sponge;
  int32_t do_vort_damp, rf_fast, hydrostatic, use_logp, grid_type;
  /* non-zero: the grid is a stretched (Schmidt-transformed) cubed sphere and the divergence damping coefficient is
   * da_min * d4_bg^(nord+1) instead of (da_min_c * d4_bg)^(nord+1).  The geometry itself arrives in fv3_griddata; a stretched
   * geometry with this flag 0 is legal.  (Takes the padding the 13 preceding int32 left: size and the offsets of the doubles
   * are unchanged.) */
  int32_t stretched_grid;
  double a_imp, beta, p_fac;
  double d2_bg, d2_bg_k1, d2_bg_k2, d4_bg, dddmp, d_con, d_ext, delt_max, ke_bg, vtdm4;
  double rf_cutoff, tau;
} fv3_acoustic_config;

/* PACE_CONSTANTS set [REF README.md:88-93] */
typedef struct {
  double radius, omega, grav, rdgas, rvgas, cp_air, dz_min, pi, seconds_per_day;
} fv3_constants;

/* DycoreState fields on the path [REF tests/main/fv3core/test_init_from_geos.py:128-199;
 * driver/pace/driver/state.py:131-139] */
typedef struct {
  fv3_field u, v, w, ua, va, uc, vc, delp, delz, pt, pe, pk, peln, pkz, q_con, omga, cappa;
  fv3_field mfxd, mfyd, cxd, cyd, diss_estd;
  fv3_field phis; /* 2-D: shape[2] == 1.  Read on the compute domain AND one halo ring (riem_solver_c's surface height on the ring of the
                   * C-grid heights): the caller fills that ring once; no halo update of the call touches phis */
} fv3_state;

int fv3_version(void);
const char *fv3_last_error(const fv3_ctx *ctx); /* ctx may be NULL: last create error */
const char *fv3_backend(void);                  /* "hip:gfx950" (product) or "hostemu" (test build) */
/* sha256 (hex, first 16 digits) of the kernel sources + headers this library was built from (pace_amd/build.py: src_hash): the counter
 * files bench.py quotes (profiles/traffic_d_sw.json, valu_d_sw.json) carry the hash of the tree they were measured on, and a line built from
 * another tree reports them as null instead of a stale number */
const char *fv3_build_id(void);

int fv3_ctx_create(fv3_ctx **out, const fv3_gridspec *spec, const fv3_griddata *grid,
                   const fv3_acoustic_config *cfg, const fv3_constants *consts, int device, int dtype);
int fv3_ctx_destroy(fv3_ctx *ctx);
/* bytes of device scratch the context owns (for memory accounting) */
int64_t fv3_ctx_scratch_bytes(const fv3_ctx *ctx);
/* device_sync: true semantics [REF .jenkins/driver_configs/baroclinic_c192_6ranks.yaml:7] */
int fv3_ctx_set_device_sync(fv3_ctx *ctx, int on);

/* ---- operators (argument order = the reference operator's __call__) ----
 * Footprints (held by tests/test_operator_footprints.py; INTEGRATION.md, "Read and write footprints"): an entry reads no pad level (level nz
 * of a cell-level field), no cube-corner halo block and no halo cell beyond what the reference operator reads; it stores into an argument
 * only on the region the reference defines that output on, levels 0 .. nz - 1 (interface fields 0 .. nz).  An output defined on the compute
 * domain + 1 ring (gz, ws, pef, pe, omga, delpc, ptc) is stored on that whole rectangle: the cube-corner halo cell in it, which has no
 * neighbour, holds no defined value.  The exceptions are stated at the entries below. */

/* CGridShallowWaterDynamics.__call__ [REF tests/savepoint/thresholds/fv_dynamics.yaml:2-75].
 * delpc / ptc are outputs (the reference returns them).  uc, vc, ua, va, ut, vt, divgd, omga, delpc, ptc are not read on entry; uc / vc /
 * ua / va are stored wherever the reference's d2a2c_vect stores them (halo rows that d_sw and the later stages read included). */
int fv3_c_sw(fv3_ctx *, const fv3_field *delp, const fv3_field *pt, const fv3_field *u, const fv3_field *v,
             const fv3_field *w, const fv3_field *uc, const fv3_field *vc, const fv3_field *ua,
             const fv3_field *va, const fv3_field *ut, const fv3_field *vt, const fv3_field *divgd,
             const fv3_field *omga, const fv3_field *delpc, const fv3_field *ptc, double dt2, void *stream);

/* UpdateGeopotentialHeightOnCGrid.__call__(dp_ref, zs, ut, vt, gz, ws, dt) (dp_ref lives in the ctx) */
int fv3_update_dz_c(fv3_ctx *, const fv3_field *zs, const fv3_field *ut, const fv3_field *vt,
                    const fv3_field *gz, const fv3_field *ws, double dt, void *stream);

/* RiemannSolverC.__call__(dt2, cappa, ptop, phis, ws, ptc, q_con, delpc, gz, pef, w3)
 * [REF tests/main/fv3core/test_config.py:13] */
int fv3_riem_solver_c(fv3_ctx *, double dt2, const fv3_field *cappa, double ptop, const fv3_field *phis,
                      const fv3_field *ws, const fv3_field *ptc, const fv3_field *q_con,
                      const fv3_field *delpc, const fv3_field *gz, const fv3_field *pef,
                      const fv3_field *w3, void *stream);

/* p_grad_c(rdxc, rdyc, uc, vc, delpc, pkc, gz, dt2) (rdxc/rdyc live in the ctx) */
int fv3_p_grad_c(fv3_ctx *, const fv3_field *uc, const fv3_field *vc, const fv3_field *delpc,
                 const fv3_field *pkc, const fv3_field *gz, double dt2, void *stream);

/* FiniteVolumeFluxPrep.__call__(uc, vc, crx, cry, xfx, yfx, ut, vt, dt)
 * [REF examples/notebooks/functions.py:877-891].  ut / vt are stored where the reference stores them: ut on i = 0 .. nx + 3 of every row
 * (vt: j = 0 .. ny + 3 of every column), on the two rows (columns) along a cube-tile edge only on the faces of crx (cry). */
int fv3_fxadv(fv3_ctx *, const fv3_field *uc, const fv3_field *vc, const fv3_field *crx, const fv3_field *cry,
              const fv3_field *xfx, const fv3_field *yfx, const fv3_field *ut, const fv3_field *vt, double dt,
              void *stream);

/* FiniteVolumeTransport.__call__(q, crx, cry, xfx, yfx, fx, fy[, mfx, mfy, mass])
 * [REF examples/notebooks/functions.py:935-951].  mfx/mfy/mass may be NULL.
 * nord < 0 or damp_c <= 1e-4 disables the del-n damping fluxes. */
int fv3_fv_tp_2d(fv3_ctx *, const fv3_field *q, const fv3_field *crx, const fv3_field *cry,
                 const fv3_field *xfx, const fv3_field *yfx, const fv3_field *fx, const fv3_field *fy,
                 const fv3_field *mfx, const fv3_field *mfy, const fv3_field *mass, int hord, int nord,
                 double damp_c, void *stream);

/* AGrid2BGridFourthOrder.__call__(qin, qout) ; replace != 0 writes qout back into qin */
int fv3_a2b_ord4(fv3_ctx *, const fv3_field *qin, const fv3_field *qout, int kstart, int nk, int replace,
                 void *stream);

/* DGridShallowWaterLagrangianDynamics.__call__ [REF tests/savepoint/thresholds/fv_dynamics.yaml:76-170;
 * tests/main/fv3core/test_config.py:14].  delpc is the work array of the divergence damping (as the reference's argument of that name): any
 * cell of it may change, and uc / vc hold work values afterwards.  delpc, crx, cry, xfx, yfx, zh, diss_est are not read
 * on entry. */
int fv3_d_sw(fv3_ctx *, const fv3_field *delpc, const fv3_field *delp, const fv3_field *pt, const fv3_field *u,
             const fv3_field *v, const fv3_field *w, const fv3_field *uc, const fv3_field *vc,
             const fv3_field *ua, const fv3_field *va, const fv3_field *divgd, const fv3_field *mfx,
             const fv3_field *mfy, const fv3_field *cx, const fv3_field *cy, const fv3_field *crx,
             const fv3_field *cry, const fv3_field *xfx, const fv3_field *yfx, const fv3_field *q_con,
             const fv3_field *zh, const fv3_field *heat_source, const fv3_field *diss_est, double dt,
             void *stream);

/* UpdateHeightOnDGrid.__call__(zs, zh, crx, cry, xfx, yfx, wsd, dt) */
int fv3_update_dz_d(fv3_ctx *, const fv3_field *zs, const fv3_field *zh, const fv3_field *crx,
                    const fv3_field *cry, const fv3_field *xfx, const fv3_field *yfx, const fv3_field *wsd,
                    double dt, void *stream);

/* RiemannSolver3.__call__(last_call, dt, cappa, ptop, zs, wsd, delz, q_con, delp, pt, zh, pe, ppe, pk3, pk, peln, w) */
int fv3_riem_solver3(fv3_ctx *, int last_call, double dt, const fv3_field *cappa, double ptop,
                     const fv3_field *zs, const fv3_field *wsd, const fv3_field *delz, const fv3_field *q_con,
                     const fv3_field *delp, const fv3_field *pt, const fv3_field *zh, const fv3_field *pe,
                     const fv3_field *ppe, const fv3_field *pk3, const fv3_field *pk, const fv3_field *peln,
                     const fv3_field *w, void *stream);

/* PK3Halo.__call__(pk3, delp, ptop, akap) and the edge_pe stencil */
int fv3_pk3_halo(fv3_ctx *, const fv3_field *pk3, const fv3_field *delp, double ptop, double akap, void *stream);
int fv3_edge_pe(fv3_ctx *, const fv3_field *pe, const fv3_field *delp, double ptop, void *stream);

/* NonHydrostaticPressureGradient.__call__(u, v, pp, gz, pk3, delp, dt, ptop, akap) */
int fv3_nh_p_grad(fv3_ctx *, const fv3_field *u, const fv3_field *v, const fv3_field *pp, const fv3_field *gz,
                  const fv3_field *pk3, const fv3_field *delp, double dt, double ptop, double akap, void *stream);

/* RayleighDamping.__call__(u, v, w, dp, pfull, dt, ptop) (dp_ref / pfull live in the ctx)
 * [REF driver/examples/configs/baroclinic_c12.yaml:73-75] */
int fv3_ray_fast(fv3_ctx *, const fv3_field *u, const fv3_field *v, const fv3_field *w, double dt, double ptop,
                 void *stream);

/* HyperdiffusionDamping.__call__(q, cd) and apply_diffusive_heating */
int fv3_del2_cubed(fv3_ctx *, const fv3_field *q, double cd, int nmax, void *stream);
int fv3_apply_diffusive_heating(fv3_ctx *, const fv3_field *delp, const fv3_field *delz, const fv3_field *cappa,
                                const fv3_field *heat_source, const fv3_field *pt, double delt_time_factor,
                                void *stream);

/* small glue stencils of dyn_core: set_gz, copy, zero, gz = zh * grav */
int fv3_set_gz(fv3_ctx *, const fv3_field *zs, const fv3_field *delz, const fv3_field *gz, void *stream);
int fv3_copy(fv3_ctx *, const fv3_field *src, const fv3_field *dst, void *stream);
int fv3_zero(fv3_ctx *, const fv3_field *dst, void *stream);
int fv3_compute_geopotential(fv3_ctx *, const fv3_field *zh, const fv3_field *gz, void *stream);

/* ---- halo exchange (HaloUpdater pack / unpack) [REF docs/util/communication.rst:43-109] ----
 * A plan is a gather list built on the host from the partitioner geometry:
 * value[dst] = sign * source[src].  The same kernel packs (source = field, dst = buffer),
 * unpacks (source = buffer) and does the device-local copy between co-resident sub-domains. */
typedef struct fv3_gather_plan fv3_gather_plan;
/* dst_off / src_off: element offsets of the (sub, j, i) column base inside the respective
 * allocation (k stride is supplied per call); n entries; nk levels are moved per entry. */
int fv3_gather_plan_create(fv3_ctx *, fv3_gather_plan **out, int64_t n, const int64_t *dst_off,
                           const int64_t *src_off, const int8_t *sign);
int fv3_gather_plan_destroy(fv3_gather_plan *);
int fv3_gather_run(fv3_ctx *, const fv3_gather_plan *, void *dst, int64_t dst_kstride, const void *src,
                   int64_t src_kstride, int nk, void *stream);

/* ---- halo updaters behind the ABI (fv3_halo_plan_create / start / wait) ----------------------------
 * One plan = one HaloUpdater of the reference [REF docs/util/communication.rst:100-109,169-176]: a list of gather
 * operations on borrowed field pointers -- copies between co-resident sub-domains, packs into and unpacks out of one
 * message buffer per peer process -- and the peers with their message sizes.  start(): pack, post every message of the
 * update (RCCL: one ncclGroupStart/End of ncclSend/ncclRecv), local copies; wait(): unpack.  With a communicator
 * the exchange runs on the context's communication stream and overlaps what the caller enqueues in between. */
typedef struct fv3_halo_plan fv3_halo_plan;
enum { FV3_HALO_LOCAL = 0, FV3_HALO_PACK = 1, FV3_HALO_UNPACK = 2 };
typedef struct {
  const fv3_gather_plan *plan;
  void *dst;           /* LOCAL / UNPACK: destination field (all sub-domains); PACK: ignored (the peer's send buffer) */
  const void *src;     /* LOCAL / PACK: source field; UNPACK: ignored (the peer's receive buffer) */
  int64_t dst_kstride; /* elements between levels of the field side(s) */
  int64_t src_kstride;
  int64_t buf_off;     /* PACK / UNPACK: element offset of this piece inside the message buffer ... */
  int64_t buf_kstride; /* ... and the elements between its levels there */
  int32_t peer;        /* PACK / UNPACK: index into the plan's peer list */
  int32_t kind;        /* FV3_HALO_LOCAL / PACK / UNPACK */
  int32_t nk;          /* levels moved per gather entry */
  int32_t reserved;
} fv3_halo_op;
typedef struct {
  int32_t rank;        /* communicator rank of the peer process */
  int32_t reserved;
  int64_t send_elems, recv_elems;
  void *send_buf, *recv_buf; /* optional caller-owned message buffers (NULL: allocated by the plan, device memory) */
} fv3_halo_peer;
int fv3_halo_plan_create(fv3_ctx *, fv3_halo_plan **out, int n_ops, const fv3_halo_op *ops, int n_peers,
                         const fv3_halo_peer *peers);
int fv3_halo_plan_start(fv3_ctx *, fv3_halo_plan *, void *stream);
int fv3_halo_plan_wait(fv3_ctx *, fv3_halo_plan *, void *stream);
int fv3_halo_plan_destroy(fv3_halo_plan *);
int fv3_halo_plan_buffer(fv3_halo_plan *, int peer_index, int recv, void **ptr, int64_t *elems);

/* Transport.  RCCL point-to-point over xGMI: the 128-byte id is made on rank 0 (fv3_comm_unique_id), distributed by the
 * launcher's own channel, and every process calls fv3_ctx_comm_init (= ncclCommInitRank) once, before its first
 * exchange; librccl.so is bound at run time.  Host-driven transport (tests, gloo): the plan packs, calls
 * fn(user, plan, 0) [post the messages], later fn(user, plan, 1) [complete them], then unpacks. */
typedef struct { char internal[128]; } fv3_nccl_id;
int fv3_rccl_available(void); /* 1 when librccl.so could be bound in this process (what every rank checks BEFORE the collective calls) */
int fv3_comm_unique_id(fv3_nccl_id *id);
int fv3_ctx_comm_init(fv3_ctx *, const fv3_nccl_id *id, int world, int rank);
int fv3_ctx_comm_destroy(fv3_ctx *);
typedef int (*fv3_xfer_fn)(void *user, fv3_halo_plan *plan, int phase);
int fv3_ctx_set_xfer(fv3_ctx *, fv3_xfer_fn fn, void *user);
/* run the exchanges on the context's second stream (default: on with a communicator, off without) */
int fv3_ctx_set_comm_stream(fv3_ctx *, int on);
/* the stream the exchanges run on when that is switched on (hipStream_t as void*), else NULL: a host-driven transport enqueues its
 * own copies there so that they stay ordered with the plan's pack / unpack kernels */
void *fv3_ctx_get_comm_stream(fv3_ctx *);

/* ---- whole acoustic call [REF AcousticDynamics.__call__; SURVEY §3.3] ----------------------------
 * Temporaries AcousticDynamics owns (allocated by the host's QuantityFactory, borrowed here). */
typedef struct {
  fv3_field gz, zh, pkc, pk3;             /* interface fields (nz+1) */
  fv3_field crx, cry, xfx, yfx;           /* Courant numbers / area fluxes of d_sw */
  fv3_field divgd, ut, vt;                /* corner divergence, contravariant C-grid winds */
  fv3_field delpc, ptc;                   /* c_sw outputs */
  fv3_field dsw_delpc;                    /* d_sw work field (its "delpc" argument) */
  fv3_field heat_source;
  fv3_field ws3, wsd, zs;                 /* 2-D */
} fv3_workspace;

/* The 11 halo updaters of AcousticDynamics + the D-grid interface synchronisation. */
enum fv3_halo_update {
  FV3_HALO_Q_CON__CAPPA = 0,
  FV3_HALO_DELP__PT,
  FV3_HALO_U__V,
  FV3_HALO_W,
  FV3_HALO_GZ,
  FV3_HALO_DIVGD,
  FV3_HALO_UC__VC,
  FV3_HALO_DELP__PT__Q_CON,
  FV3_HALO_ZH,
  FV3_HALO_PKC,
  FV3_HALO_HEAT_SOURCE,
  FV3_HALO_INTERFACE_U__V,
  FV3_HALO_COUNT
};
/* Host-provided transport: phase 0 = start (pack + post), 1 = wait (complete + unpack), both
 * enqueued on `stream`.  Returns 0 on success.  The library never moves halos on its own. */
typedef int (*fv3_halo_fn)(void *user, int update /* fv3_halo_update */, int phase, void *stream);

/* The updaters as plans, indexed by fv3_halo_update: fv3_acoustic_step then needs no callback (halo = NULL) and no
 * host code runs between its operators. */
int fv3_ctx_set_halo_plans(fv3_ctx *, fv3_halo_plan *const *plans, int n);

/* n_split acoustic sub-steps (+ the once-per-call diffusive heating when d_con > 1e-5);
 * timestep = dt_atmos / k_split, n_map = 1..k_split.  halo == NULL: the registered plans (fv3_ctx_set_halo_plans).
 * The flux accumulators of the state (mfxd, mfyd, cxd, cyd) hold this call's fluxes on return [dyn_core.F90: emptied at the start of
 * every call]; the library zeroes each array in full the first time the context sees its pointer and afterwards has the first
 * sub-step store into the cells d_sw writes ("Flux accumulators").  With a halo callback the first sub-step asks for
 * FV3_HALO_ZH where the reference's sequence updates gz (the heights of a call are computed straight into zh). */
int fv3_acoustic_step(fv3_ctx *, const fv3_state *state, const fv3_workspace *work, double timestep, int n_map,
                      fv3_halo_fn halo, void *halo_user, void *stream);

/* ---- SURVEY §8f-3 (next row): sub-cycled tracer advection ---------------------------------------------------
 * TracerAdvection.__call__(tracers, dp1, mfxd, mfyd, cxd, cyd) [REF examples/notebooks/functions.py:916-951,
 * 1037-1044; savepoint Tracer2D1L, tests/savepoint/thresholds/fv_dynamics.yaml:328-360].  The one global quantity of
 * the operator is the Courant-number bound: fv3_tracer_2d_1l_cmax returns this process's maximum of
 * max(|cx|, |cy|) + 1 - sin_sg5 (it synchronises the stream), the host all-reduces it (MAX) and passes
 * n_split = (int)(1 + cmax).  cxd / cyd / mfxd / mfyd are scaled by 1 / n_split in place and dp1 ends as the air mass
 * before the last sub-cycle, like the reference's fields (Tracer2D1L-Out).  tracer_halo (may be NULL when n_split == 1):
 * the halo plan of the tracers, run between sub-cycles.  hord: 5 / 6, or 8 = PPM with the fast monotone constraint
 * (hord_tr of the reference configs [REF driver/examples/configs/baroclinic_c12.yaml:60]). */
int fv3_tracer_2d_1l_cmax(fv3_ctx *, const fv3_field *cxd, const fv3_field *cyd, double *cmax, void *stream);
int fv3_tracer_2d_1l(fv3_ctx *, int n_tracers, const fv3_field *const *tracers, const fv3_field *dp1,
                     const fv3_field *mfxd, const fv3_field *mfyd, const fv3_field *cxd, const fv3_field *cyd,
                     int n_split, int hord, fv3_halo_plan *tracer_halo, void *stream);

/* LagrangianToEulerian (the vertical remap that closes DynamicalCore.step_dynamics) [REF driver/pace/driver/driver.py:494-504,
 * 639-644; savepoint Remapping: tests/savepoint/thresholds/fv_dynamics.yaml:227-326; kord_tm -9, kord_mt / kord_tr / kord_wz 9,
 * consv_te 0: driver/examples/configs/baroclinic_c12.yaml:45,65-68].  In place: pt (the loop's theta_v / pkz form), delp, delz,
 * u, v, w and the tracers go from the Lagrangian layers (interfaces = pe / peln as the last acoustic sub-step left them,
 * pe's one-cell halo ring by edge_pe) to the Eulerian ones ak + bk * ps; pe, peln, pk, pkz and ps (2-D) are rebuilt.
 * Configuration of the reference configs: non-hydrostatic, T_v remapped in log(p), kord 9 everywhere, moist-cappa pkz with
 * the given cappa field, no energy fixer, no saturation adjustment, omga untouched; nz >= 5.  The vertical filling of negative
 * tracer means that the reference runs at the end of the tracer part (`fill: true`) is its own entry, fv3_fillz, called right
 * after this one with the remapped tracers and delp. */
int fv3_remap(fv3_ctx *, int n_tracers, const fv3_field *const *tracers, const fv3_field *pt, const fv3_field *delp,
              const fv3_field *delz, const fv3_field *peln, const fv3_field *pe, const fv3_field *pk, const fv3_field *pkz,
              const fv3_field *u, const fv3_field *v, const fv3_field *w, const fv3_field *cappa, const fv3_field *ps,
              const fv3_field *wsd, void *stream);

/* fillz (FV3 fv_fill.F90, default form; pyFV3 FillNegativeTracerValues: the end of the tracer part of LagrangianToEulerian with
 * `fill: true` [REF driver/examples/configs/baroclinic_c12.yaml:56]).  In place on the compute cells 1..nx x 1..ny, levels
 * 0 .. nz-1 of every sub-domain; halo cells and the pad level nz of the tracers are neither read nor written; dp (after the remap:
 * the Eulerian delp) is only read.  Per column and tracer, 0-based, km = nz, in the build's Real, every product, quotient and sum
 * rounded on its own:
 *   top       q[0] < 0: q[1] = q[1] + (q[0] * dp[0]) / dp[1], q[0] = 0 (does not set zfix);
 *   interior  k = 1 .. km-2 in increasing order, q[k] < 0: zfix; where q[k-1] > 0, dq = min(q[k-1] * dp[k-1], -q[k] * dp[k]) moves
 *             from level k-1 to k (q[k-1] - dq / dp[k-1], q[k] + dq / dp[k]); where q[k] is still < 0 and q[k+1] > 0,
 *             dq = min(q[k+1] * dp[k+1], -q[k] * dp[k]) moves from level k+1 to k; level k+1 is then visited with what is left;
 *   bottom    k = km-1, q[k] < 0 and q[k-1] > 0: zfix; dup = min(-q[k] * dp[k], q[k-1] * dp[k-1]) moves from level k-1 to k (a
 *             negative bottom layer under a non-positive one is left alone);
 *   non-local where zfix: dm[k] = q[k] * dp[k] for k = 1 .. km-1, sum0 = sum dm[k], sum1 = sum max(0, dm[k]) (increasing k, from 0);
 *             where sum0 > 0: q[k] = max(0, ((sum0 / sum1) * dm[k]) / dp[k]) for k = 1 .. km-1 (level 0 is not touched).
 * Comparisons are plain IEEE (-0.0 and NaN take no branch; min(a, b) = a < b ? a : b; max(0, x) = x < 0 ? 0 : x in the quotient,
 * x > 0 ? x : 0 in sum1).  A column of a tracer without a negative value is not written at all.  The tracers are taken four to a
 * launch, sharing the reads of dp.  FV3_ERR_ARG (a message, nothing launched): n_tracers < 0, a null list with n_tracers > 0, a
 * null or 2-D dp, a tracer that does not match the context layout, dp among the tracers, a tracer given twice.
 * FV3_ERR_UNSUPPORTED: nz < 2.  n_tracers == 0: FV3_OK, nothing launched. */
int fv3_fillz(fv3_ctx *, int n_tracers, const fv3_field *const *tracers, const fv3_field *dp, void *stream);

/* ---- the thermodynamic bookends of DynamicalCore.step_dynamics (fv3_thermo.hip) ---------------------------------------------
 * state.pt is a temperature (K) before and after a model step [REF driver/pace/driver/driver.py:494-504, 639-644]; the acoustic
 * loop, the tracer advection and the remap work on T_v / pkz.  Both entries work on the compute cells 1..nx x 1..ny, levels
 * 0 .. nz-1 of every sub-domain, in the build's Real, every product and quotient rounded on its own, left to right; halo cells,
 * the pad level nz and the fields that are only read are never written.  exp / log are the calls of fv3_remap's kernels.
 *   rrg = (Real)(-rdgas / grav), zvir = (Real)(rvgas / rdgas - 1), fac = (1 + zq) * (1 - q_con) with zq = zvir * qvapor, or
 *   zq = 0 where qvapor is NULL (bitwise what a qvapor field of zeros gives).  q_con and cappa are fields here: fv3_moist_cv
 *   (below) derives them from the water species.
 *
 * fv3_pt_from_temperature, the preamble of fv_dynamics (pt: T in, the loop's form out; pkz: out):
 *   tv = pt * fac;  pz = exp(cappa * log(rrg * delp / delz * tv));  pkz = pz;  pt = tv / pz
 *
 * fv3_temperature_from_pt, the last-step conversion of the remap and the omga / ps diagnoses (pt: the loop's form in, T out):
 *   recompute_pkz == 0:  tv = pt * pkz                       (FV3's own form: valid where pkz belongs to pt, i.e. after a remap)
 *   recompute_pkz == 1:  tv = pt * exp(cappa / (1 - cappa) * log(rrg * delp / delz * pt));
 *                        pkz = exp(cappa * log(rrg * delp / delz * tv))     (pkz is rebuilt from the state, as fv3_remap does)
 *   pt = tv / fac;  omga = delp / delz * w  where omga is not NULL;  ps = pe[.., nz]  where ps is not NULL (a 2-D field)
 *
 * FV3_ERR_ARG (a message, nothing launched, no field changed): a null context, a null or wrongly shaped field (ps must be 2-D,
 * every other field 3-D), recompute_pkz other than 0 / 1, pt / pkz / omga / ps given twice, one of them also given as a field
 * that is only read (delp, delz, q_con, cappa, qvapor, w, pe). */
int fv3_pt_from_temperature(fv3_ctx *, const fv3_field *pt, const fv3_field *pkz, const fv3_field *delp, const fv3_field *delz,
                            const fv3_field *q_con, const fv3_field *cappa, const fv3_field *qvapor, void *stream);
int fv3_temperature_from_pt(fv3_ctx *, const fv3_field *pt, const fv3_field *pkz, const fv3_field *delp, const fv3_field *delz,
                            const fv3_field *q_con, const fv3_field *cappa, const fv3_field *qvapor, const fv3_field *w,
                            const fv3_field *omga, const fv3_field *pe, const fv3_field *ps, int recompute_pkz, void *stream);

/* ---- moist thermodynamics: q_con and cappa from the water species (fv3_moist.hip, fv3_remap.hip) --------------------------------
 * FV3 derives the condensate mixing ratio q_con and the moist R / c_p (cappa) from the water species with moist_cv (fv_mapz.F90),
 * once in the preamble of fv_dynamics and again inside every remap, after the tracers are remapped and filled and before pkz is
 * rebuilt.  The nwat = 6 formula, in the build's Real, every sum, product and quotient rounded on its own in the order written:
 *   qv = qvapor;  ql = qliquid + qrain;  qs = (qice + qsnow) + qgraupel
 *   q_con = ql + qs
 *   cvm   = (((1 - (qv + q_con)) * cv_air + qv * cv_vap) + ql * c_liq) + qs * c_ice
 *   cappa = rdgas / (rdgas + cvm / (1 + zvir * qv))
 * cv_air = (Real)(cp_air - rdgas), zvir = (Real)(rvgas / rdgas - 1), rdgas = (Real)rdgas from the context's constants; cv_vap, c_liq
 * and c_ice (J/kg/K) travel with the species.  A species given as NULL is a field of zeros, bitwise; qvapor may not be NULL. */
typedef struct {
  const fv3_field *qvapor, *qliquid, *qrain, *qice, *qsnow, *qgraupel;
  double cv_vap, c_liq, c_ice;
} fv3_water;

/* fv3_moist_cv: q_con, cappa and (where cvm is not NULL) cvm on the compute cells 1..nx x 1..ny, levels 0 .. nz-1 of every
 * sub-domain; halo cells, the pad level and the species are never written.
 *
 * fv3_pt_from_temperature_moist: the preamble of fv_dynamics with moist_cv inside the cell.  q_con and cappa (both out) are formed
 * from the species, then the formulas of fv3_pt_from_temperature with qvapor = water->qvapor (pt: T in, the loop's form out; pkz:
 * out).  Bit for bit fv3_moist_cv followed by fv3_pt_from_temperature.
 *
 * FV3_ERR_ARG (a message that names the field, nothing launched, no field changed): a null context, a null fv3_water, a null
 * qvapor, a null or wrongly shaped field or species, an output given twice, an output that is also a field that is only read. */
int fv3_moist_cv(fv3_ctx *, const fv3_water *water, const fv3_field *q_con, const fv3_field *cappa, const fv3_field *cvm,
                 void *stream);
int fv3_pt_from_temperature_moist(fv3_ctx *, const fv3_field *pt, const fv3_field *pkz, const fv3_field *delp,
                                  const fv3_field *delz, const fv3_field *q_con, const fv3_field *cappa, const fv3_water *water,
                                  void *stream);

/* fv3_remap_moist: fv3_remap with moist_cv where FV3 has it.  The T_v kernel at the top reads the incoming cappa; the fields are
 * remapped as by fv3_remap; with fill != 0 the negative means of all tracers are then filled in the vertical with the Eulerian
 * layer thickness (bitwise fv3_fillz on the final delp); the closing column kernel forms q_con and cappa per level from the remapped
 * and filled species, stores them (q_con: out; cappa: in, then out) and uses the new cappa for
 * pkz = exp(cappa * log(rrg * delp / delz * tv)), pt = tv / pkz.  The species are the fields that get remapped: each one given must
 * be one of `tracers` (the same storage).  Everything but q_con, cappa, pkz and pt is bitwise what fv3_remap (+ fv3_fillz) gives.
 * FV3_ERR_ARG (a message, nothing launched, no field changed): what fv3_remap and fv3_moist_cv reject, a species that is not among
 * the tracers, a tracer given twice, q_con given as another argument.  FV3_ERR_UNSUPPORTED: nz < 5. */
int fv3_remap_moist(fv3_ctx *, int n_tracers, const fv3_field *const *tracers, const fv3_field *pt, const fv3_field *delp,
                    const fv3_field *delz, const fv3_field *peln, const fv3_field *pe, const fv3_field *pk, const fv3_field *pkz,
                    const fv3_field *u, const fv3_field *v, const fv3_field *w, const fv3_field *cappa, const fv3_field *q_con,
                    const fv3_field *ps, const fv3_field *wsd, const fv3_water *water, int fill, void *stream);

/* ---- negative water species (fv3_negadj.hip) ----------------------------------------------------------------------------------
 * neg_adj3 (FV3 fv_sg.F90, the non-hydrostatic form; pyFV3 AdjustNegativeTracerMixingRatio), which fv_dynamics runs between the last
 * remap and CubedToLatLon when nwat = 6: a negative condensate is paid for out of another phase with the latent heat booked on the
 * temperature, negative vapour is repaid from the layer below.  In place on the compute cells 1..nx x 1..ny, levels 0 .. nz-1
 * (km = nz) of every sub-domain; halo cells and the pad level are neither read nor written; pt is the temperature in K (as
 * fv3_temperature_from_pt leaves it); dp = delp is only read; q_con and cappa are not touched (the next preamble rebuilds them).
 * In the build's Real, every sum, product and quotient rounded on its own in the order written.  Constants, formed in double and
 * cast once: cv_air = cp_air - rdgas (the context's constants); cv_vap, c_liq, c_ice of the fv3_water; d0_vap = cv_vap - c_liq;
 * lv00 = hlv - (cv_vap - c_liq) * t_ice; dc_ice = c_liq - c_ice; li00 = hlf - (c_liq - c_ice) * t_ice, with the latent heats of
 * vaporisation and fusion hlv, hlf (J/kg) and the freezing point t_ice (K) of the fv3_latent.
 *   per cell, from the cell's incoming values:
 *     q_liq = max(0, ql + qr);  q_sol = max(0, qi + qs)                                       (graupel is not part of q_sol)
 *     cpm   = (((1 - ((qv + q_liq) + q_sol)) * cv_air + qv * cv_vap) + q_liq * c_liq) + q_sol * c_ice
 *     lcpk  = (lv00 + d0_vap * pt) / cpm;  icpk = (li00 + dc_ice * pt) / cpm
 *   then in this order, each test seeing the results of the ones before it:
 *     qi < 0:  qs = qs + qi;  qi = 0
 *     qs < 0:  qg = qg + qs;  qs = 0
 *     qg < 0:  qr = qr + qg;  pt = pt - qg * icpk;  qg = 0
 *     qr < 0:  ql = ql + qr;  qr = 0
 *     ql < 0:  qv = qv + ql;  pt = pt - ql * lcpk;  ql = 0
 *   per column, after the cell step of all its levels, vapour only:
 *     k = 0 .. km-2 in increasing order, qv[k] < 0:  qv[k+1] = qv[k+1] + (qv[k] * dp[k]) / dp[k+1];  qv[k] = 0
 *     bottom, qv[km-1] < 0 and qv[km-2] > 0:  dq = min(-qv[km-1] * dp[km-1], qv[km-2] * dp[km-2]);
 *                                             qv[km-2] = qv[km-2] - dq / dp[km-2];  qv[km-1] = qv[km-1] + dq / dp[km-1]
 * Comparisons are plain IEEE (-0.0 and NaN take no branch); max(0, x) = x > 0 ? x : 0; min(a, b) = a < b ? a : b.  A value is stored
 * only where a branch changed it: a column in which no comparison is true is not written at all.
 * FV3_ERR_ARG (a message that names the field, nothing launched, no field changed): a null context, fv3_water or fv3_latent; any of the
 * six species NULL (this entry needs all six); a null or wrongly shaped field; a species given twice; pt or delp among the species;
 * pt == delp.  FV3_ERR_UNSUPPORTED: nz < 2. */
typedef struct {
  double hlv, hlf, t_ice;
} fv3_latent;
int fv3_neg_adj3(fv3_ctx *, const fv3_water *water, const fv3_latent *latent, const fv3_field *pt, const fv3_field *delp,
                 void *stream);

/* ---- saturation adjustment (fv3_satadj.hip, fv3_satadj.h; the fused form in fv3_remap.hip) ----------------------------------------
 * fv_sat_adj (FV3 fv_cmp.F90, the non-hydrostatic form), which FV3 runs inside every remap when do_sat_adj is set: after the remap and
 * the fill, before moist_cv and pkz.  Phase changes between the six species, the latent heat booked on the temperature.  Restated
 * from the Fortran; not built: the energy-fixer branch (consv_te = 0), the out_dt tendency, the cloud fraction (do_qa / qa).
 * In the build's Real, every sum, product and quotient rounded on its own in the order written, left to right; exp and log are the
 * build's; min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b, of three: min(min(a, b), c), max(max(a, b), c); dim(a, b) = max(a - b, 0).
 * Constants, formed in double and cast once: cv_air .. li00 as in fv3_neg_adj3; zvir = rvgas / rdgas - 1, rvgas, grav (the context's);
 * tice = t_ice; tice0 = t_ice - 0.01; t_wfr = t_ice - 40; lat2 = (hlv + hlf)^2; mdt: the remap interval (s); sdt = 0.5 mdt; dt_bigg = mdt;
 *   fac_X = 1 - exp(-mdt / tau_X) for X = i2s, r2g, l2r, smlt;  fac_X = 1 - exp(-sdt / tau_X) for X = v2l, imlt;
 *   fac_l2v = min(sat_adj0, 1 - exp(-sdt / tau_l2v)).
 * Shorthands: cvm = ((mc_air + qv * cv_vap) + q_liq * c_liq) + q_sol * c_ice;  heat(s, L): cvm again, then pt1 = pt1 + s * L / cvm;
 *   lat: lhl = lv00 + d0_vap * pt1; lhi = li00 + dc_ice * pt1; lcp2 = lhl / cvm; icp2 = lhi / cvm.
 * Per cell (tv = T (1 + zvir qv)(1 - q_con) in and out; dp = delp; delz):
 *    1  q_liq = ql + qr; q_sol = (qi + qs) + qg; qpz = q_liq + q_sol; pt1 = tv / ((1 + zvir * qv) * (1 - qpz)); qpz = qpz + qv;
 *       den = dp / (-grav * delz); mc_air = (1 - qpz) * cv_air; cvm; lat
 *    2  qi < 0: qs += qi; qi = 0
 *    3  qi > 1e-8 and pt1 > tice: sink = min(qi, fac_imlt * (pt1 - tice) / icp2); qi -= sink; tmp = min(sink, dim(ql_mlt, ql));
 *       ql += tmp; qr += sink - tmp; q_liq += sink; q_sol -= sink; heat(-sink, lhi); lat
 *    4  qs < 0: qg += qs; qs = 0;  else qg < 0: tmp = min(-qg, max(0, qs)); qg += tmp; qs -= tmp
 *    5  ql < 0: tmp = min(-ql, max(0, qr)); ql += tmp; qr -= tmp;  else qr < 0: tmp = min(-qr, max(0, ql)); ql -= tmp; qr += tmp
 *    6  dtmp = (tice - 48) - pt1; ql > 0 and dtmp > 0: sink = min(ql, ql * dtmp * 0.125, dtmp / icp2); ql -= sink; qi += sink;
 *       q_liq -= sink; q_sol += sink; heat(sink, lhi); lat
 *    7  (wqsat, dq2dt) = wqs2(pt1, den); dq0 = (qv - wqsat) / (1 + lcp2 * dq2dt);
 *       dq0 > 0: src = min(sat_adj0 * dq0, max(ql_gen - ql, fac_v2l * dq0));
 *       else factor = -min(1, fac_l2v * 10 * (1 - qv / wqsat)); src = -min(ql, factor * dq0);
 *       qv -= src; ql += src; q_liq += src; heat(src, lhl); lat
 *    8  last_step only: step 7 again with src = dq0 where dq0 > 0
 *    9  dtmp = t_wfr - pt1; as step 6
 *   10  tc = tice0 - pt1; ql > 0 and tc > 0: sink = 3.3333e-10 * dt_bigg * (exp(0.66 * tc) - 1) * den * ql * ql;
 *       sink = min(ql, tc / icp2, sink); the updates of step 6; heat(sink, lhi); lat
 *   11  dtmp = (tice - 0.1) - pt1; qr > 1e-7 and dtmp > 0: x = dtmp * 0.025; tmp = min(1, x * x) * qr; sink = min(tmp, fac_r2g * dtmp / icp2);
 *       qr -= sink; qg += sink; q_liq -= sink; q_sol += sink; heat(sink, lhi); lat
 *   12  dtmp = pt1 - (tice + 0.1); qs > 1e-7 and dtmp > 0: x = dtmp * 0.1; tmp = min(1, x * x) * qs; sink = min(tmp, fac_smlt * dtmp / icp2);
 *       tmp = min(sink, dim(qs_mlt, ql)); qs -= sink; ql += tmp; qr += sink - tmp; q_liq += sink; q_sol -= sink; heat(-sink, lhi)
 *   13  ql > ql0_max: sink = fac_l2r * (ql - ql0_max); qr += sink; ql -= sink.  Then lat; tcp2 = lcp2 + icp2
 *   14  src = 0;  pt1 < t_sub: src = dim(qv, 1e-6);
 *       else pt1 < tice0: (qsi, dqsdt) = iqs2(pt1, den); dq = qv - qsi; sink = sat_adj0 * dq / (1 + tcp2 * dqsdt);
 *         pidep = qi > 1e-8 ? sdt * dq * 349138.78 * exp(0.875 * log(qi * den)) / (qsi * den * lat2 / (0.0243 * rvgas * pt1 * pt1) + 4.42478e4) : 0;
 *         dq > 0: tmp = tice - pt1; qi_crt = qi_gen * min(qi_lim, 0.1 * tmp) / den; src = min(sink, max(qi_crt - qi, pidep), tmp / tcp2);
 *         else pidep = pidep * min(1, dim(pt1, t_sub) * 0.2); src = max(pidep, sink, -qi);
 *       qv -= src; qi += src; q_sol += src; heat(src, lhl + lhi)
 *   15  tv = pt1 * (1 + zvir * qv) * (1 - (q_liq + q_sol))
 *   16  qg < 0: tmp = min(-qg, max(0, qi)); qg += tmp; qi -= tmp
 *   17  qim = qi0_max / den; qi > qim: sink = fac_i2s * (qi - qim); qi -= sink; qs += sink
 * The q_con and cappa that are stored are moist_cv of the final species (the formulas above), not the sums step 15 forms in passing.
 * Saturation tables (FV3 qs_init; four arrays of 2621 entries, entry n = 1 .. 2621 at T_n = (t_ice - 160) + 0.1 (n - 1), formed in
 * double on the host and cast): tablew[n] = e00 * exp((dc_vap * log(T_n / t_ice) + lv0 * (T_n - t_ice) / (T_n * t_ice)) / rvgas) with
 * e00 = 611.21, dc_vap = (cv_vap + rvgas) - c_liq, lv0 = hlv - dc_vap * t_ice; table2[n]: for n <= 1600 the same with dc_vap + dc_ice
 * and lv0 + li00, above that tablew[n], entries 1600 and 1601 replaced by 0.25 * (t[n-1] + 2 t[n] + t[n+1]) of the unsmoothed values;
 * desw[n] = max(0, tablew[n+1] - tablew[n]) of the cast entries, the last entry repeating the one before it; des2 likewise.
 * Lookup: ap1 = min(2621, 10 * dim(T, tice - 160) + 1); it = floor(ap1); es = tab[it] + (ap1 - it) * des[it]; qs = es / (rvgas * T * den);
 * it = max(1, floor(ap1 - 0.5)); dqdt = 10 * (des[it] + (ap1 - it) * (des[it+1] - des[it])) / (rvgas * T * den).  wqs2: tablew, desw; iqs2: table2, des2.
 * The tables are built by the context's first adjusting call, in device memory the context owns; a later call allocates nothing. */
typedef struct {
  double tau_i2s, tau_v2l, tau_l2v, tau_imlt, tau_r2g, tau_smlt, tau_l2r; /* time scales (s): 1000, 150, 300, 600, 900, 900, 900 */
  double ql_gen, qi_gen, qi_lim, ql_mlt, qs_mlt, ql0_max, qi0_max;       /* 1e-3, 1.82e-6, 1, 2e-3, 1e-6, 2e-3, 1e-4 */
  double sat_adj0, t_sub;                                                /* 0.9, 184 */
} fv3_sat_params;

/* fv3_sat_adj: the adjustment alone, in place on the compute cells 1..nx x 1..ny of levels kmp .. nz-1, where kmp is the first level
 * whose reference mid-pressure pfull_k = (ph_{k+1} - ph_k) / log(ph_{k+1} / ph_k), ph = ak + bk * 1e5, exceeds 10 hPa (formed in double
 * from the context's ak / bk; fv3_sat_adj_level0 returns it).  tv (in, out), the six species (in, out); q_con, cappa, pkz (out):
 * moist_cv of the adjusted species and pkz = exp(cappa * log(rrg * delp / delz * tv)); delp and delz are only read.  Nothing is read or
 * written above kmp, in the halo or on the pad level.
 * FV3_ERR_ARG (a message that names the field, nothing launched, no field changed): a null context, fv3_water, fv3_latent or
 * fv3_sat_params; any species NULL; a null or wrongly shaped field; a field given twice (among tv, delp, delz, q_con, cappa, pkz and the
 * species); mdt <= 0; last_step other than 0 / 1; a tau_* that is not positive.
 * fv3_sat_adj_tables: tablew, table2, desw, des2 one after the other as the kernels hold them, widened to double; n must be 4 * 2621;
 * FV3_ERR_ARG before the context's first adjusting call (the tables are made of that call's constants). */
int fv3_sat_adj(fv3_ctx *, const fv3_water *water, const fv3_latent *latent, const fv3_sat_params *params, const fv3_field *tv,
                const fv3_field *delp, const fv3_field *delz, const fv3_field *q_con, const fv3_field *cappa, const fv3_field *pkz,
                double mdt, int last_step, void *stream);
int fv3_sat_adj_level0(fv3_ctx *, int *kmp);
int fv3_sat_adj_tables(fv3_ctx *, double *out, long n);

/* fv3_remap_moist_sat: fv3_remap_moist with the adjustment where FV3 has it, inside the closing column kernel: on the levels
 * kmp .. nz-1 the remapped and filled species and the remapped T_v go through the cell step above before moist_cv and pkz are formed;
 * no extra pass over the fields.  Bit for bit fv3_remap_moist, then fv3_sat_adj on tv = pt * pkz, then pt = tv / pkz (to that end the
 * kernel forms the unadjusted pkz of such a cell first and starts from tv = (T_v / pkz) * pkz).  All six species are needed.
 * FV3_ERR_ARG: what fv3_remap_moist and fv3_sat_adj reject. */
int fv3_remap_moist_sat(fv3_ctx *, int n_tracers, const fv3_field *const *tracers, const fv3_field *pt, const fv3_field *delp,
                        const fv3_field *delz, const fv3_field *peln, const fv3_field *pe, const fv3_field *pk, const fv3_field *pkz,
                        const fv3_field *u, const fv3_field *v, const fv3_field *w, const fv3_field *cappa, const fv3_field *q_con,
                        const fv3_field *ps, const fv3_field *wsd, const fv3_water *water, int fill, const fv3_latent *latent,
                        const fv3_sat_params *params, double mdt, int last_step, void *stream);

/* CubedToLatLon (the last operator of fv_dynamics: FV3 fv_grid_utils.F90 c2l_ord4 / c2l_ord2; pyFV3 CubedToLatLon, savepoint
 * FVDynamics-Out ua / va [REF tests/savepoint/thresholds/fv_dynamics.yaml]).  D-grid u, v -> ua, va on the compute cells in earth
 * coordinates (eastward, northward).  order: c2l_ord, 4 (the reference's default) or 2.  a11 .. a22: the cell-centre rotation
 * terms (2-D fields, shape[2] == 1; GridData a11 .. a22).  Order 4 reads u at j-1 .. j+2 and v at i-1 .. i+2: the caller updates
 * the D-grid halo of u, v before the call.  Levels 0 .. nz-1; nothing outside the compute cells of ua / va is written. */
int fv3_cubed_to_latlon(fv3_ctx *, int order, const fv3_field *u, const fv3_field *v, const fv3_field *ua, const fv3_field *va,
                        const fv3_field *a11, const fv3_field *a12, const fv3_field *a21, const fv3_field *a22, void *stream);

/* ---- physics coupling: a source of tendencies (fv3_hs.hip) and their application to the D-grid state (fv3_updphys.hip) ----------
 *
 * Held-Suarez (1994) forcing [Held & Suarez, Bull. Amer. Meteor. Soc. 75, 1825-1830]; the defaults of the paper are
 * sigma_b = 0.7, k_f = 1 / 86400 1/s, k_a = 1 / (40 * 86400), k_s = 1 / (4 * 86400), delta_t_y = 60 K, delta_theta_z = 10 K,
 * p0 = 1e5 Pa, kappa = 2 / 7, t_min = 200 K. */
typedef struct fv3_held_suarez {
  double sigma_b, k_f, k_a, k_s, delta_t_y, delta_theta_z, p0, kappa, t_min;
} fv3_held_suarez;

/* fv3_held_suarez_tend: u_dt, v_dt, t_dt on the compute cells of levels 0 .. nz-1 from ua, va (eastward / northward cell-centre
 * winds), pt (temperature, K), delp (Pa) and lat (2-D field, radians).  Stateless: pe(0) = ptop, pe(k+1) = pe(k) + delp(k),
 * ps = pe(nz), p = (pe(k) + pe(k+1)) / 2, sigma = p / ps;
 *   s = max(0, (sigma - sigma_b) / (1 - sigma_b)),  k_v = k_f s,  k_T = k_a + (k_s - k_a) s cos^4(lat),
 *   T_eq = max(t_min, (315 - delta_t_y sin^2(lat) - delta_theta_z ln(p / p0) cos^2(lat)) (p / p0)^kappa),
 *   u_dt = -k_v / (1 + dt k_v) ua, v_dt likewise from va, t_dt = -k_T / (1 + dt k_T) (pt - T_eq)   (implicit in dt; dt = 0: explicit).
 * Nothing outside the compute cells of the outputs is written, no input is written.  FV3_ERR_ARG: an output that aliases an
 * input or another output, dt < 0 or not finite, parameters outside 0 <= sigma_b < 1, p0 > 0, k_* >= 0. */
int fv3_held_suarez_tend(fv3_ctx *, const fv3_held_suarez *params, const fv3_field *ua, const fv3_field *va, const fv3_field *pt,
                         const fv3_field *delp, const fv3_field *lat, const fv3_field *u_dt, const fv3_field *v_dt, const fv3_field *t_dt,
                         double ptop, double dt, void *stream);

/* fv3_apply_tendencies (FV3 fv_update_phys: the temperature update and update_dwinds_phys; pyFV3 ApplyPhysicsToDycore):
 *   pt += dt t_dt on the compute cells;  with V = u_dt vlon + v_dt vlat (Cartesian tendency at a cell centre)
 *   u(i,j) += dt (V(i,j-1) + V(i,j)) / 2 . es(i,j)  for i = 1..nx, j = 1..ny+1,
 *   v(i,j) += dt (V(i-1,j) + V(i,j)) / 2 . ew(i,j)  for i = 1..nx+1, j = 1..ny,
 * on a tile-edge face with the averaged vector interpolated along the edge, (1 - w) Vbar_f + w Vbar_f' (f' = the neighbouring
 * face towards the middle of the edge).  2-D fields (GridData of the same names): vlon_x, vlon_y / vlat_x .. vlat_z the east /
 * north unit vectors of the cell centres, es_* / ew_* the unit tangents of the x- / y-faces, ev_um / ev_up (ev_vm / ev_vp) the
 * weight w of a south / north (west / east) tile-edge face whose f' has index - 1 / + 1, zero on every other face.  The caller
 * updates one halo cell of u_dt, v_dt (as scalars: the components are geographic) before the call; cube-corner halo cells are not
 * read.  Levels 0 .. nz-1.  FV3_ERR_ARG: a tendency that aliases u / v / pt, dt not finite. */
int fv3_apply_tendencies(fv3_ctx *, const fv3_field *u, const fv3_field *v, const fv3_field *pt, const fv3_field *u_dt, const fv3_field *v_dt,
                         const fv3_field *t_dt, const fv3_field *vlon_x, const fv3_field *vlon_y, const fv3_field *vlat_x,
                         const fv3_field *vlat_y, const fv3_field *vlat_z, const fv3_field *es_x, const fv3_field *es_y, const fv3_field *es_z,
                         const fv3_field *ew_x, const fv3_field *ew_y, const fv3_field *ew_z, const fv3_field *ev_um, const fv3_field *ev_up,
                         const fv3_field *ev_vm, const fv3_field *ev_vp, double dt, void *stream);

/* ---- dry convective adjustment of the sponge layers (fv3_subgridz.hip) ------------------------------------------------------------
 * FV3 fv_sg.F90, subroutine fv_subgrid_z in its non-hydrostatic form; pyFV3 DryConvectiveAdjustment, which the reference driver runs
 * after every step_dynamics when fv_sg_adj > 0 and whose wind tendencies fv3_apply_tendencies then applies.  Restated (the source is
 * not in the reference tree: unpinned).  Levels are 0-based from the top; everything in the build's Real, every
 * sum, product and quotient rounded on its own in the order written; min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b,
 * dim(a, b) = max(a - b, 0), comparisons plain IEEE.
 *
 * params: dt (s), tau (s, the namelist's fv_sg_adj), t_min, t_max (K), kbot (levels the operator works on; clipped to nz).  Formed in
 * double and cast once: rdt = 1 / dt, fra = dt / tau; grav, g2 = 0.5 grav, cv_air = cp_air - rdgas (the context's constants),
 * xvir = rvgas / rdgas - 1 (0 when water is NULL); cv_vap, c_liq, c_ice of the fv3_water.  ustar2 = 1e-4, ri_max = 1, ri_min = 0.25.
 *
 * Working copy on levels 0 .. kbot-1: u0 = ua, v0 = va, w0 = w, t0 = pt, q0_i = q_i.  Per level (an absent species is 0):
 *   q_liq = ql + qr;  q_sol = (qi + qs) + qg
 *   cvm   = (((1 - ((qv + q_liq) + q_sol)) * cv_air + qv * cv_vap) + q_liq * c_liq) + q_sol * c_ice          (dry: cv_air)
 *   qcon  = (((ql + qi) + qs) + qr) + qg                                                                     (dry: 0)
 *   tvol(k) = gz[k] + 0.5 * ((u0 * u0 + v0 * v0) + w0 * w0)
 * Three passes n = 1, 2, 3 with ratio = (Real)n / (Real)3.  At the start of a pass, from the current working copy, gzh = 0 and for
 * k = kbot-1 down to 0:  gz[k] = gzh - g2 * delz[k];  te[k] = cvm[k] * t0[k] + tvol(k);  gzh = gzh - grav * delz[k].
 * Then for k = kbot-1 down to 1 (upper level m = k-1, lower level k), each pair seeing what the pair below it left:
 *   tv1 = t0[m] * ((1 + xvir * qv[m]) - qcon[m]);  tv2 likewise at k;  pt1 = tv1 / pkz[m];  pt2 = tv2 / pkz[k]
 *   ri  = ((gz[m] - gz[k]) * (pt1 - pt2)) / ((0.5 * (pt1 + pt2)) * (((u0[m] - u0[k])^2 + (v0[m] - v0[k])^2) + ustar2))
 *   if (tv1 > t_max && tv1 > tv2) ri = 0;  else if (tv2 < t_min) ri = min(ri, 0.1)
 *   pm = delp[k] / (peln[k+1] - peln[k]);  ri_ref = min(ri_max, ri_min + ((ri_max - ri_min) * dim(400e2, pm)) / 200e2)
 *   k == 1: ri_ref = 4 ri_ref;  k == 2: ri_ref = 2 ri_ref;  k == 3: ri_ref = 1.5 ri_ref
 *   r = 1 - max(0, ri / ri_ref);  mc = ri < ri_ref ? (((ratio * delp[m]) * delp[k]) / (delp[m] + delp[k])) * (r * r) : 0
 *   if (mc > 0): for X in every tracer, u0, v0, te, w0:  h0 = mc * (X[k] - X[m]);  X[m] = X[m] + h0 / delp[m];  X[k] = X[k] - h0 / delp[k]
 *                for kk in (m, k): qcon[kk], cvm[kk] from the mixed species;  t0[kk] = (te[kk] - tvol(kk)) / cvm[kk]
 * (te keeps its mixed value within a pass.)  After the third pass, in a column where some mc > 0 occurred: if fra < 1 every working
 * value becomes X = X_in + (X - X_in) * fra; on levels 0 .. kbot-1  u_dt = rdt * (u0 - ua), v_dt = rdt * (v0 - va), pt = t0, w = w0,
 * q_i = q0_i.  A column without any mc > 0 is not stored (pt, w and the tracers stay bitwise) and gets zero tendencies; so do levels
 * kbot .. nz-1 of every column.  u_dt, v_dt are assigned on the compute cells of levels 0 .. nz-1; nothing else outside levels
 * 0 .. kbot-1 of the compute cells of pt, w and the tracers is written.  q_con, cappa and pkz of the state are not updated.
 *
 * water (NULL: dry): species that are given must be among `tracers`; they are mixed by the main walk, the other tracers by a second
 * kernel from the stored mc.  work: scratch fields of the context's 3-D layout, 2 + n_tracers of them, and 3 more when a tracer is
 * not a water species (t0, w0, one copy per tracer, mc of the three passes); u_dt and v_dt hold u0, v0 during the call.
 * FV3_ERR_ARG (a message that names the field, nothing launched, no field changed): a null context or params; a null or wrongly
 * shaped field (every 3-D field of the layout has the nz + 1 levels peln needs); a written field (pt, w, a tracer, u_dt, v_dt, a
 * work field) that is also given as another argument; a species that is not among the tracers; dt <= 0 or not finite; tau <= 0;
 * kbot < 0; too few work fields.  kbot < 3: FV3_OK, the tendencies are zeroed and nothing else happens. */
typedef struct fv3_subgridz_params {
  double dt, tau, t_min, t_max;
  int kbot;
} fv3_subgridz_params;
int fv3_subgrid_z(fv3_ctx *, const fv3_subgridz_params *, const fv3_water *water /* NULL: dry */, int n_tracers,
                  const fv3_field *const *tracers, const fv3_field *ua, const fv3_field *va, const fv3_field *w, const fv3_field *pt,
                  const fv3_field *delp, const fv3_field *delz, const fv3_field *peln, const fv3_field *pkz, const fv3_field *u_dt,
                  const fv3_field *v_dt, int n_work, const fv3_field *const *work, void *stream);

/* ---- driver diagnostics (fv3_diag.hip): what the driver stores every output_frequency steps ------------------------------
 * [REF driver/pace/driver/diagnostics.py].  Neither entry allocates: the caller owns `out`, a contiguous device array in the
 * build's Real.  Neither reads a halo cell or the pad level.
 *
 * fv3_diag_pack: the compute box i = 1..ni, j = 1..nj, levels k0 .. k0+nk-1 of every sub-domain of `src` -> out[t][k][j][i]
 * (i fastest).  ni is nx or nx+1, nj is ny or ny+1 (the staggered end belongs to the variable: u has nj = ny+1, v ni = nx+1);
 * the level range lies in [0, nz] for a 3-D field (an interface field: nk = nz+1), a 2-D field (shape[2] == 1) takes k0 = 0,
 * nk = 1; a level slice is nk = 1.  A null out, another ni / nj, a level range outside the field or
 * out_elems != n_sub * nk * nj * ni: FV3_ERR_ARG, a message, nothing launched.  One launch for all sub-domains. */
int fv3_diag_pack(fv3_ctx *, const fv3_field *src, int ni, int nj, int k0, int nk, void *out, long out_elems, void *stream);

/* fv3_diag_column_integral: out[t][j][i] = rgrav * sum_{k = 0}^{nz-1} q * delp on the compute cells (rgrav = 1 / grav of the
 * context's constants; kg/m^2 for a mixing ratio).  The products are rounded, then added in increasing k in Real, the sum is
 * multiplied by rgrav once: the result is fixed bitwise.  out_elems must be n_sub * ny * nx. */
int fv3_diag_column_integral(fv3_ctx *, const fv3_field *q, const fv3_field *delp, void *out, long out_elems, void *stream);

/* ---- per-operator timing (HIP events on the operators' stream) --------------------------------- */
enum fv3_op {
  FV3_OP_C_SW = 0,
  FV3_OP_UPDATE_DZ_C,
  FV3_OP_RIEM_SOLVER_C,
  FV3_OP_P_GRAD_C,
  FV3_OP_D_SW,
  FV3_OP_UPDATE_DZ_D,
  FV3_OP_RIEM_SOLVER3,
  FV3_OP_PK3_HALO,
  FV3_OP_NH_P_GRAD,
  FV3_OP_RAY_FAST,
  FV3_OP_DIFFUSIVE_HEATING,
  FV3_OP_GLUE,
  FV3_OP_HALO,
  FV3_OP_COUNT
};
int fv3_ctx_set_profiling(fv3_ctx *, int on); /* 1: record an event pair around every operator of fv3_acoustic_step; 2: around d_sw only; 0: off */
const char *fv3_op_name(int op);
/* accumulated milliseconds and call counts per fv3_op (arrays of FV3_OP_COUNT); waits for the events */
int fv3_profile_read(fv3_ctx *, double *ms_sum, int64_t *calls, int reset);

/* Device self-test of the hand-written fp64 arithmetic of the Riemann solvers (no reference counterpart; tests/test_device_math.py).
 * x, y, out: device pointers to n doubles.  which 0: out = x / y by the solvers' division sequence; 1: their log; 2: their exp;
 * 3: round trip through the 80 accumulation-register slots of one wave (n = 80 * 64).  fp64 values in both builds. */
int fv3_selftest_math(fv3_ctx *, int which, const double *x, const double *y, double *out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FV3_MI355X_H */
