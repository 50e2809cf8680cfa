/*
 * roms_hip.h -- C ABI of the MI355X-native ROMS nonlinear 3-D time-stepping
 * hot path (libroms_hip.so).
 *
 * The reference has no FFI; its seam is the Fortran module-procedure name
 * `CALL X(ng, tile)` used by ROMS/Nonlinear/main3d.F:307-814 and
 * ROMS/Nonlinear/initial.F:337-571.  Each entry point below replaces the body
 * of one such procedure (the file:line it replaces is cited on the
 * declaration).  The ISO_C_BINDING interface block a maintainer adds on the
 * Fortran side is in roms_trunk_mgh_amd/fortran/roms_hip_mod.F90 and
 * INTEGRATION.md.
 *
 * Conventions
 *   - plain C: ints, doubles, pointers; no C++/torch types.
 *   - every entry returns int: 0 = ROMS NoError; non-zero = error, mapped by
 *     the Fortran shim to exit_flag 8 (algorithm) or 2 (communication), the
 *     codes of ROMS/Modules/mod_scalars.F:523-532.  The library never aborts.
 *   - host arrays stay owned by the caller (Fortran `allocate`); the library
 *     owns device mirrors and device scratch (the `_tile` routines' automatic
 *     IminS:ImaxS work arrays).
 *   - array layout = the reference's: column-major, i fastest, common
 *     horizontal extents LBi:UBi,LBj:UBj for every field of a tile.
 */
#ifndef ROMS_HIP_H
#define ROMS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Field identifiers and shapes                                        */
/* ------------------------------------------------------------------ */
enum roms_kind {
  K_2D = 0, K_2D_T2, K_2D_T3, K_2D_NT,
  K_3DR, K_3DW, K_3DR_T2, K_3DW_T2, K_3DW_NAT, K_4DT, K_3DR_NT, K_3DW_T3
};

enum roms_field_id {
#define ROMS_FIELD(name, kind, owner) FID_##name,
#include "roms_fields.def"
#undef ROMS_FIELD
  FID_COUNT
};

/* All module arrays of one tile (host pointers in the oracle, device pointers
 * inside the library). */
typedef struct roms_fields {
#define ROMS_FIELD(name, kind, owner) double *name;
#include "roms_fields.def"
#undef ROMS_FIELD
} roms_fields_t;

/* ------------------------------------------------------------------ */
/* Limits and codes of the run-time parameters (roms_params_t)         */
/* ------------------------------------------------------------------ */
#define ROMS_MAXN   64     /* max vertical levels held in the param block   */
#define ROMS_MAXNT  16     /* max tracers                                   */
#define ROMS_MAXFAST 256   /* max 2*ndtfast                                 */

/* Tracer advection scheme codes = the logical records of T_ADV
 * (mod_param.F:382-394). */
enum roms_adv {
  ADV_C2 = 0, ADV_C4, ADV_A4, ADV_U3, ADV_SU3, ADV_SPLINES, ADV_MPDATA, ADV_HSIMT
};
/* Pressure-gradient algorithm (the CPP choice of ROMS/Nonlinear/prsgrd.F:16-26): DJ_GRADPS = prsgrd32.h (the three
 * application headers of BASELINE.json define it), none of the options = prsgrd31.h (standard density Jacobian, the
 * reference's default), WJ_GRADP = prsgrd31.h with the weighted Jacobian of Song (1998). */
enum roms_pgf { PGF_DJ_GRADPS = 0, PGF_STANDARD = 1, PGF_WJ_GRADP = 2, PGF_PJ_GRADP = 3 /* prsgrd40.h: finite-volume pressure Jacobian */ };
/* Lateral boundary condition codes supported on this path (the logical records of T_LBC, mod_param.F:348-363).
 * A periodic direction (E-W) has LBC_PERIODIC on both of its sides; a physical edge (any of the four) takes, per
 * variable (roms_params_t.lbc): closed, gradient, clamped, radiation (implicit upstream, zetabc.F:108 /
 * u2dbc_im.F:135 / v2dbc_im.F:136 / u3dbc_im.F:131 / v3dbc_im.F:97 / t3dbc_im.F:128 and the other edges' blocks; no
 * nudging, RADIATION_2D off) for every variable; Chapman implicit for zeta (zetabc.F:193); Flather for ubar and
 * vbar (u2dbc_im.F:214, v2dbc_im.F:216 for the normal component,
 * [radiation + nudging towards the boundary data, "RadNud", for every variable: e.g. t3dbc_im.F:138-152, :183-188] the Chapman-type rule of u2dbc_im.F:912 /
 * v2dbc_im.F:886 for the tangential one); then the corner rule (zetabc.F:699).  Anything else is refused by every
 * entry that applies conditions; N-S periodic grids are refused. */
enum roms_lbc {
  LBC_PERIODIC = 0, LBC_CLOSED = 1, LBC_GRADIENT = 2, LBC_CLAMPED = 3, LBC_CHAPMAN_IMPLICIT = 4, LBC_FLATHER = 5,
  LBC_RADIATION = 6, LBC_RADIATION_NUDGING = 7,
  LBC_CHAPMAN_EXPLICIT = 8,          /* "Che", free surface only: zetabc.F:175-190 */
  LBC_SHCHEPETKIN = 9,               /* "Shc", ubar / vbar only: u2dbc_im.F:288-362, v2dbc_im.F:290-364 (bry_val = the boundary data) */
  LBC_REDUCED = 10                   /* "Red", ubar / vbar only: reduced physics (pressure gradient, Coriolis, surface and
                                      * bottom stress), u2dbc_im.F:392-432, v2dbc_im.F:394-436 */
};
/* rows of roms_params_t.lbc = the state variables of LBC(:, isFsur / isUbar / isVbar / isUvel / isVvel / isTvar, ng) */
enum roms_lbc_var { LBV_ZETA = 0, LBV_UBAR, LBV_VBAR, LBV_U, LBV_V, LBV_T, LBV_COUNT };
enum roms_lbc_side { LBS_WEST = 0, LBS_EAST, LBS_SOUTH, LBS_NORTH };
/* Momentum advection, roms_params_t.uv_adv: 0 = no UV_ADV; otherwise ROMS_UV_ADV(h, v) with the horizontal and the
 * vertical scheme the application header selects.  1 = ROMS_UV_ADV(ROMS_UVH_U3, ROMS_UVV_C4W) is the reference's
 * default: third-order upstream horizontally (rhs3d.F:706-730 ...), fourth-order centred vertical flux with the
 * fourth-order averaged W (:1177-1256), fourth-order centred in step2d (step2d_LF_AM3.h:1077-1256).
 *   ROMS_UVH_C2  UV_C2ADVECTION  second-order centred (rhs3d.F:605-656; in step2d step2d_LF_AM3.h:1026-1076)
 *   ROMS_UVH_C4  UV_C4ADVECTION  fourth-order centred (rhs3d.F:685-705, :761-778, :829-849, :902-919)
 *   ROMS_UVV_C2  UV_C2ADVECTION  (:1079-1107, :1330-1361)
 *   ROMS_UVV_C4  UV_C4ADVECTION  weights 9/32, 1/32 on the velocity, the two-point sum of W (:1108-1176, :1362-1433)
 *   ROMS_UVV_SPLINES  UV_SADVECTION  conservative parabolic splines (:1016-1078, :1267-1329)
 * The six pairs the reference can be compiled to are accepted -- (U3, C4W), (U3, SPLINES), (C2, C2), (C2, SPLINES),
 * (C4, C4), (C4, SPLINES) -- and every other value is refused by roms_hip_rhs3d_tile, roms_hip_rhs3d, roms_hip_step2d
 * and roms_hip_step2d_loop (error text "uv_adv").  step2d takes the C2 form exactly when h = ROMS_UVH_C2. */
enum roms_uv_hadv { ROMS_UVH_U3 = 0, ROMS_UVH_C2 = 1, ROMS_UVH_C4 = 2 };
enum roms_uv_vadv { ROMS_UVV_C4W = 0, ROMS_UVV_C2 = 1, ROMS_UVV_C4 = 2, ROMS_UVV_SPLINES = 3 };
#define ROMS_UV_ADV(h, v) (1 | ((h) << 4) | ((v) << 8))
#define ROMS_UV_HADV(uv_adv) (((uv_adv) >> 4) & 15)      /* the two schemes of a valid non-zero uv_adv */
#define ROMS_UV_VADV(uv_adv) (((uv_adv) >> 8) & 15)
/* roms_params_t.gls_stability */
enum roms_gls_stab { GLS_GALPERIN = 0, GLS_KANTHA_CLAYSON = 1, GLS_CANUTO_A = 2, GLS_CANUTO_B = 3 };

/* ------------------------------------------------------------------ */
/* The three structs of the boundary.  Each is declared once, as an    */
/* X-macro table beside this header (roms_bounds.def, roms_params.def, */
/* roms_step_idx.def: one entry per member, with the member's          */
/* documentation); the ctypes mirror and the tests read the same       */
/* tables.                                                             */
/* ------------------------------------------------------------------ */
#define ROMS_MEMBER(type, name)             type name;
#define ROMS_MEMBER_A(type, name, n)        type name[n];
#define ROMS_MEMBER_A2(type, name, n1, n2)  type name[n1][n2];

/* Tile bounds: every integer of ROMS/Include/set_bounds.h:20-79 and ROMS/Include/tile.h:21-45, plus
 * DOMAIN(ng)%*_Edge(tile) (ROMS/Modules/mod_param.F:286-323) and the grid sizes. */
typedef struct roms_bounds {
#include "roms_bounds.def"
} roms_bounds_t;

/* Run-time parameters (mod_scalars.F, mod_param.F) and option switches; every member is documented in the table. */
typedef struct roms_params {
#include "roms_params.def"
} roms_params_t;

/* Time-level indices = mod_stepping.F (nstp,nnew,nrhs,kstp,krhs,knew) and
 * mod_scalars.F (iic, iif, ntfirst, PREDICTOR_2D_STEP); see
 * main3d.F:189-191 and main3d.F:597-662.  All 1-based as in Fortran. */
typedef struct roms_step_idx {
#include "roms_step_idx.def"
} roms_step_idx_t;

/* Parameters of the NPZD_POWELL ecosystem model (roms_hip_set_biology): a table of its own, roms_bio.def, so that the
 * three structs above keep their layout. */
typedef struct roms_bio_powell {
#include "roms_bio.def"
} roms_bio_powell_t;

/* Parameters of the BIO_FENNEL ecosystem model (roms_hip_set_biology): roms_bio_fennel.def.  The CPP options of the
 * reference are 0/1 members (bio_sediment, denitrification, oxygen, carbon, bulk_fluxes).  The device side of the model
 * is not built yet (see BIOLOGY below): no entry takes this block. */
typedef struct roms_bio_fennel {
#include "roms_bio_fennel.def"
} roms_bio_fennel_t;

#undef ROMS_MEMBER
#undef ROMS_MEMBER_A
#undef ROMS_MEMBER_A2

/* ------------------------------------------------------------------ */
/* Library life cycle                                                  */
/* ------------------------------------------------------------------ */
/* Replaces nothing; called once after ROMS_initialize (nl_roms.h:60-231).
 * nccl_unique_id: 128-byte ncclUniqueId shared by all ranks, or NULL (one tile, or a multi-tile run whose
 * halos go through roms_hip_set_halo_relay).  One tile WITH an id = loopback: the periodic wrap of the tile
 * is sent through RCCL to the tile itself and every kernel takes its multi-tile branch (same results; lets a
 * one-GPU box execute the RCCL transport). */
int roms_hip_init(int rank, int ntileI, int ntileJ, int device_id,
                  const void *nccl_unique_id);
int roms_hip_finalize(void);
/* 128-byte id for roms_hip_init, generated on rank 0 (ncclGetUniqueId). */
int roms_hip_get_unique_id(void *out128);

/* BOUNDS(ng)%...(tile): get_bounds.F:738 (get_tile), :1009 (var_bounds).
 * May be called again in a live context (a re-grid; the tiling of roms_hip_init stays).  It forgets everything that
 * has the old extents: every field registration and device mirror, the library-kept defaults, the source table, the
 * climatology, the averages, the floats, the tidal strips, the records of roms_hip_set_data_record, the row table of the grid metrics, the halo neighbour table and message
 * plan, and the captured LOOP_2D graphs.  The caller then sets the parameters, registers and uploads every field
 * and hands sources / climatology / averages / floats / tides / data records over again, as after roms_hip_init; the context then computes
 * what a fresh one does, bit for bit. */
int roms_hip_set_bounds(const roms_bounds_t *b);
int roms_hip_set_params(const roms_params_t *p);

/* Register the host address (c_loc) of one module array; allocates its
 * device mirror.  n_doubles is checked against the shape implied by kind. */
int roms_hip_register_field(int field_id, double *host_ptr, long n_doubles);
/* Host <-> device copies of one field (whole array). */
int roms_hip_sync_to_device(int field_id);
int roms_hip_sync_to_host(int field_id);
int roms_hip_sync_all_to_device(void);
int roms_hip_sync_all_to_host(void);
/* Asynchronous snapshot for the unchanged output / wrt_his / wrt_rst (ROMS/Nonlinear/output.F:123-208):
 * begin() copies the n listed fields aside on the device (ordered with the kernels already issued) and starts
 * their transfer to the registered host arrays on a second stream, then returns; the step loop may go on and
 * overwrite the fields.  end() waits for the transfer: the host arrays then hold the fields as they were at
 * begin().  One snapshot in flight at a time; the host arrays must not be read or written in between. */
int roms_hip_snapshot_begin(const int *field_ids, int n);
int roms_hip_snapshot_end(void);
/* Device address of a field mirror (for zero-copy consumers); NULL if none.  The grid-metric arrays are taken to
 * be constant between uploads (roms_hip_row_metrics_state below): a consumer that WRITES one of them through this
 * pointer must upload or re-register the field afterwards. */
double *roms_hip_device_ptr(int field_id);
int roms_hip_device_synchronize(void);
const char *roms_hip_last_error(void);

/* ------------------------------------------------------------------ */
/* Hot-path entry points -- one per reference module procedure         */
/* ------------------------------------------------------------------ */
/* set_massflux(ng,tile,model)      ROMS/Nonlinear/set_massflux.F:28  */
int roms_hip_set_massflux(const roms_step_idx_t *s);
/* rho_eos(ng,tile,model)           ROMS/Nonlinear/rho_eos.F:47       */
int roms_hip_rho_eos(const roms_step_idx_t *s);
/* omega(ng,tile,model)             ROMS/Nonlinear/omega.F:28         */
int roms_hip_omega(const roms_step_idx_t *s);
/* set_zeta(ng,tile)                ROMS/Nonlinear/set_zeta.F:25      */
int roms_hip_set_zeta(const roms_step_idx_t *s);
/* set_depth(ng,tile,model)         ROMS/Nonlinear/set_depth.F:33     */
int roms_hip_set_depth(const roms_step_idx_t *s);
/* Informational: how the barotropic kernel reads the fifteen grid-metric arrays (pm, pn, on_u, om_v, fomn, dndx,
 * dmde, pmon_r, pnom_r, pmon_p, pnom_p, om_r, on_r, om_p, on_p).  0 = not examined since their last upload;
 * 1 = all of them are independent of i on this tile and its ghost columns (checked bit for bit on the device over
 * Istr-NghostPoints : Iend+NghostPoints: a zonally uniform grid) and
 * the kernel takes them from a per-row table; 2 = they are not, and it reads the arrays; 3 = as 1, and the resting
 * depth h and the viscosity coefficients visc2_r, visc2_p are independent of i as well (flat or zonally uniform
 * bathymetry) and come from the table too.  Same results in every case. */
int roms_hip_row_metrics_state(void);
/* ini_zeta(ng,tile,model)          ROMS/Nonlinear/ini_fields.F:780
 * ini_fields(ng,tile,model)        ROMS/Nonlinear/ini_fields.F:27
 * The first-step initialisation of main3d.F:269-283 (ini_zeta, set_depth, ini_fields, in this order): other
 * time levels loaded from the initial state, MASKING multiplies, lateral boundary conditions, ubar/vbar = the
 * vertical means of u/v, Zt_avg1 = the initial free surface.  Uses s->kstp, knew, nstp, nnew. */
int roms_hip_ini_zeta(const roms_step_idx_t *s);
int roms_hip_ini_fields(const roms_step_idx_t *s);
/* rhs3d(ng,tile) -> pre_step3d, prsgrd, t3dmix2, t3dmix4, rhs3d_tile, uv3dmix2, uv3dmix4 (each mixing call
 * under its switch ts_dif2 / ts_dif4 / uv_vis2 / uv_vis4)
 *                                  ROMS/Nonlinear/rhs3d.F:25         */
int roms_hip_rhs3d(const roms_step_idx_t *s);
/* Fewest levels: roms_hip_pre_step3d, roms_hip_rhs3d_tile (so roms_hip_rhs3d) and roms_hip_step3d_t refuse N < 4
 * ("needs N >= 4 levels"): their columns are walked with the levels k-1 .. k+2 held in registers, which the
 * fourth-order vertical stencils need from N = 4 on.  roms_hip_prsgrd, roms_hip_wvelocity and the two GLS entries
 * refuse N < 3.  Every other entry runs from N = 3 on (tests/test_gpu_wide.py, shape "thin"). */
/* the pieces of rhs3d, exported for per-kernel parity tests */
int roms_hip_pre_step3d(const roms_step_idx_t *s);  /* pre_step3d.F:39   */
int roms_hip_prsgrd(const roms_step_idx_t *s);      /* prsgrd32.h:40     */
int roms_hip_t3dmix2(const roms_step_idx_t *s);     /* t3dmix2_geo.h:23  */
int roms_hip_rhs3d_tile(const roms_step_idx_t *s);  /* rhs3d.F:174       */
int roms_hip_uv3dmix2(const roms_step_idx_t *s);    /* uv3dmix2_s.h:42; with uv_vis2 = 2 uv3dmix2_geo.h:42 */
int roms_hip_t3dmix4(const roms_step_idx_t *s);     /* t3dmix4_s.h:23, t3dmix4_geo.h:23 (TS_DIF4) */
int roms_hip_uv3dmix4(const roms_step_idx_t *s);    /* uv3dmix4_s.h:43; with uv_vis4 = 2 uv3dmix4_geo.h:42 (UV_VIS4; three ghost points, inp_par.F:268) */
/* step2d(ng,tile)                  ROMS/Nonlinear/step2d_LF_AM3.h:18 */
int roms_hip_step2d(const roms_step_idx_t *s);
/* step3d_uv(ng,tile)               ROMS/Nonlinear/step3d_uv.F:27     */
int roms_hip_step3d_uv(const roms_step_idx_t *s);
/* step3d_t(ng,tile)                ROMS/Nonlinear/step3d_t.F:40      */
int roms_hip_step3d_t(const roms_step_idx_t *s);

/* Per-step physics between the hot kernels, main3d.F:388-430:
 * bulk_flux(ng,tile)               ROMS/Nonlinear/bulk_flux.F:46     */
int roms_hip_bulk_flux(const roms_step_idx_t *s);
/* set_vbc(ng,tile)                 ROMS/Nonlinear/set_vbc.F:34       */
int roms_hip_set_vbc(const roms_step_idx_t *s);
/* lmd_vmix(ng,tile) = lmd_vmix_tile + lmd_skpp + lmd_finish   ROMS/Nonlinear/lmd_vmix.F:37 */
int roms_hip_lmd_vmix(const roms_step_idx_t *s);
/* LMD_BKPP: the K-profile bottom boundary layer, lmd_bkpp(ng,tile), ROMS/Nonlinear/lmd_bkpp.F:44 -> lmd_bkpp_tile
 * (:95, the text :233-804), which lmd_vmix calls between lmd_skpp and lmd_finish (lmd_vmix.F:83-89).  Built as the file
 * is (its own SASHA) with RI_SPLINES and SALINITY, MASKING at run time; not built: LMD_SHAPIRO, the form without
 * RI_SPLINES, LIMIT_VDIFF / LIMIT_VVISC, the average avghbbl.
 *
 * roms_hip_set_kpp(1, hbbl) switches it on: the library allocates hbbl (double), kbbl and ksbl (int) of mod_mixing.F on
 * (LBi:UBi, LBj:UBj); hbbl is set from the host array (a restart: get_state.F reads it, and the depth of the previous
 * step enters bl_dpth at lmd_bkpp.F:243) or, with NULL, to zero as mod_mixing.F leaves it.  From then on
 * roms_hip_lmd_vmix runs lmd_skpp, lmd_bkpp and lmd_finish in the reference's order, with bc_r2d_tile(hbbl) and its
 * exchange (lmd_bkpp.F:577-586) beside those of hsbl; the per-step call stays the one roms_hip_lmd_vmix.
 * roms_hip_set_kpp(0, NULL) releases the arrays and roms_hip_lmd_vmix launches what it launched before;
 * roms_hip_set_bounds drops them.  Refused by name, leaving the library as it was: a call before bounds / params, a
 * value other than 0 / 1, NAT < 2 or no salinity.
 *
 * roms_hip_get_kpp copies "hbbl" (n doubles), "kbbl" or "ksbl" (n ints; ksbl as lmd_skpp.F:653-658, :787 leave it, 0
 * included) to host memory, ordered after the kernels issued; n = the points of (LBi:UBi, LBj:UBj) is checked.  wrt_rst.F
 * writes hbbl: the host fetches it here. */
int roms_hip_set_kpp(int lmd_bkpp, const double *hbbl);
int roms_hip_get_kpp(const char *name, void *host, long n);
/* LMD_DDMIX: the double-diffusive mixing of the KPP interior, lmd_vmix.F:360-430 (salt fingering and diffusive
 * convection from the density ratio Rrho = alfaobeta * dT / dS of t(nstp); constants of mod_scalars.F:1553-1577), with
 * alfaobeta = Tcof / Scof of every level out of rho_eos (rho_eos.F:427-465 nonlinear, :782-797 linear).
 *
 * roms_hip_set_ddmix(1) switches it on: the library allocates alfaobeta of mod_mixing.F on (LBi:UBi, LBj:UBj, 0:N), zero
 * as mod_mixing.F leaves it (level 0 is never written; the value of rho-level k sits at index k, as in the reference).
 * From then on roms_hip_rho_eos stores it on IstrT:IendT, JstrT:JendT and roms_hip_lmd_vmix adds nu_ddt to Akt(itemp) and
 * nu_dds to Akt(isalt) at the interior W-levels before the boundary layers match to them.  The reference exchanges
 * alfaobeta (rho_eos.F:499-503, :538-544); its only reader, lmd_vmix_tile, reads interior points, so the library does not:
 * the array is defined on the computed range only.  roms_hip_set_ddmix(0) releases the array and both entries launch what
 * they launched before; roms_hip_set_bounds drops it.  Independent of roms_hip_set_kpp.  Refused by name, leaving the
 * library as it was: a call before bounds / params, a value other than 0 / 1, NAT < 2 or no salinity (the block reads
 * t(isalt) unconditionally).  roms_hip_get_kpp("alfaobeta", host, n) copies it out, n = points x (N+1) doubles; refused
 * while the option is off. */
int roms_hip_set_ddmix(int lmd_ddmix);
/* ana_srflux(ng,tile,model)        ROMS/Functionals/ana_srflux.h:2, the ALBEDO branch (:120-150) the BENCHMARK
 * application uses: shortwave radiation from the zenith angle at (lonr, latr) for the day of the year and the
 * hour that caldate (ROMS/Utility/dateclock.F:73) returns for tdays(ng) -- the host passes those two numbers --
 * with the cloud and water-vapour corrections from cloud, Tair, Hair.  Writes srflx. */
int roms_hip_ana_srflux(double yday, double hour);
/* gls_prestep(ng,tile)             ROMS/Nonlinear/gls_prestep.F:23   (main3d.F:567, after rhs3d)
 * gls_corstep(ng,tile)             ROMS/Nonlinear/gls_corstep.F:27   (main3d.F:793, after omega and before step3d_t)
 * with tkebc_tile (tkebc_im.F:50: closed and gradient edges).  GLS_MIXING applications only: these two replace
 * lmd_vmix as the source of Akv / Akt.
 * my25_prestep(ng,tile)            ROMS/Nonlinear/my25_prestep.F:23  (main3d.F:565)
 * my25_corstep(ng,tile)            ROMS/Nonlinear/my25_corstep.F:27  (main3d.F:791)
 * MY25_MIXING applications bind the same two entries with roms_params_t.gls_mixing = 2. */
int roms_hip_gls_prestep(const roms_step_idx_t *s);
int roms_hip_gls_corstep(const roms_step_idx_t *s);
/* BIOLOGY: biology(ng,tile)        ROMS/Nonlinear/biology.F:35, called between gls_corstep and step3d_t
 * (main3d.F:795-797).  Built: NPZD_POWELL, npzd_powell_tile (ROMS/Nonlinear/Biology/npzd_Powell.h:91-661) with the
 * default, strictly monotone end conditions of the sinking reconstruction; CONST_PAR at run time.  The routine never
 * looks at rmask (land columns are computed as the reference computes them), stores t(:,:,:,nnew,idbio) on
 * Istr:Iend, Jstr:Jend only and exchanges nothing: step3d_t does afterwards.  Not built: the other models (ids below,
 * each refused by name), the LINEAR_CONTINUATION / NEUMANN end conditions, FLOAT_BIOLOGY, the TL / AD twins.
 *
 * roms_hip_set_biology(model, par, nbytes): model = ROMS_BIO_NONE drops the setting (par may be NULL, nbytes is not
 * read); ROMS_BIO_NPZD_POWELL takes par = a roms_bio_powell_t of nbytes = sizeof(roms_bio_powell_t) bytes.  Refused by
 * name, leaving the previous setting in force: a call before bounds / params, a model that is not built or unknown,
 * another nbytes, an idbio entry outside NAT+1 .. NT or repeated, BioIter < 0, a sinking speed < 0.  BioIter = 0 is
 * accepted and roms_hip_biology then returns at once (npzd_Powell.h:180).  roms_hip_set_bounds drops the setting.
 *
 * ROMS_BIO_FENNEL (fennel.h:243-1577, pCO2_water :1913-2372) is NOT built on the device: the library refuses it by
 * name like the other models.  Its parameter block, roms_bio_fennel_t above, is defined so that hosts, the Python
 * mirror and the tests agree on it already.  Options without a member there will not be built with it: PO4, RIVER_DON,
 * TALK_NONCONSERV, DIAGNOSTICS_BIO, pCO2_RZ, RW14_OXYGEN_SC, OCMIP_OXYGEN_SC, RW14_CO2_SC, PCO2AIR_DATA,
 * PCO2AIR_SECULAR, the Newton solver of pCO2_water, LINEAR_CONTINUATION / NEUMANN.
 *
 * roms_hip_biology(s) uses s->nstp and s->nnew; refused before roms_hip_set_biology ("biology is not switched on") and
 * for N < 4.  Timer entry: "biology". */
enum roms_bio_model {
  ROMS_BIO_NONE = 0, ROMS_BIO_NPZD_POWELL = 1, ROMS_BIO_NPZD_FRANKS = 2, ROMS_BIO_NPZD_IRON = 3, ROMS_BIO_FENNEL = 4,
  ROMS_BIO_NEMURO = 5, ROMS_BIO_ECOSIM = 6, ROMS_BIO_HYPOXIA_SRM = 7, ROMS_BIO_RED_TIDE = 8
};
int roms_hip_set_biology(int model, const void *par, long nbytes);
int roms_hip_biology(const roms_step_idx_t *s);
/* wetdry(ng,tile,Tindex,.TRUE.)    ROMS/Nonlinear/wetdry.F:17 -> wetdry_ini_tile (:395): the initial wet/dry masks
 * from zeta, ubar, vbar of time level Tindex = s->kstp (initial.F:438-466; WET_DRY applications).  The per-call
 * update wetdry_tile (:93) runs inside roms_hip_step2d. */
int roms_hip_wetdry(const roms_step_idx_t *s);
/* The source table SOURCES(ng) of mod_sources.F:56-80 with LuvSrc or LwSrc (roms_params_t.point_sources bits 0, 1):
 * Isrc, Jsrc (grid indices of the u- or v-face, or of the cell), Dsrc (0.0 = u-face, 1.0 = v-face, 2.0 = cell centre:
 * LwSrc), Qbar(Nsrc) (m3/s), Qsrc(Nsrc,N) = Qbar * Qshape as set_data.F:136-143 leaves it, Tsrc(Nsrc,N,NT) and
 * LtracerSrc(NT); Fortran element order.  Call it after every set_data that changes them (the arrays are copied; a
 * few kB).  The entries that consume it: step2d (step2d_LF_AM3.h:2484-2502; LwSrc: the free surface of the source
 * cells), step3d_uv (step3d_uv.F:971-995), pre_step3d (pre_step3d.F:530-553), step3d_t (step3d_t.F:734-799; LwSrc:
 * :1136-1158, :1331-1360), omega (LwSrc: omega.F:165-190), wetdry (wetdry.F:307-320, :511-524).  A source of a kind
 * whose bit of point_sources is off is not looked at. */
int roms_hip_set_sources(int Nsrc, const int *Isrc, const int *Jsrc, const double *Dsrc, const double *Qbar,
                         const double *Qsrc, const double *Tsrc, const int *LtracerSrc);
/* Nudging towards a climatology: the run-time switches LnudgeM2CLM, LnudgeM3CLM, LnudgeTCLM of a roms_*.in with the
 * members of CLIMA(ng) (mod_clima.F:190-261) they read.  No CPP option; IMPLICIT_NUDGING is not built.
 *   LnudgeTCLM[NT] = LtracerCLM(itrc,ng).and.LnudgeTCLM(itrc,ng) as 0 / 1; NTCLM = the number of set flags, and the
 *   compact index ic of a nudged tracer counts them in the order of itrc (step3d_t.F:1551-1560).
 *   Array extents are the host's: M2nudgcof, ubarclm, vbarclm (LBi:UBi,LBj:UBj); M3nudgcof, uclm, vclm
 *   (LBi:UBi,LBj:UBj,N); Tnudgcof, tclm (LBi:UBi,LBj:UBj,N,NTCLM).  Coefficients in 1/s.  Ghost points (periodic images
 *   and the points of neighbour tiles included) must be filled: the momentum terms average the coefficient over the
 *   two rho-points of a face.
 * The arrays are copied to device arrays of the library.  The entries that consume them:
 *   step3d_t     t(nnew) += dt * Tnudgcof * (tclm - t(nnew)) on IstrR:IendR, JstrR:JendR, after t3dbc_tile and before
 *                the land/sea mask and the exchange (step3d_t.F:1551-1584)
 *   rhs3d_tile   ru, rv(nrhs) += 1/4 (c(i-1)+c(i)) om_u on_u (Hz(i-1)+Hz(i)) (uclm - u(nrhs)) and the v form, after
 *                the Coriolis and curvilinear terms, before the advection (rhs3d.F:567-594)
 *   step2d       the same with M2nudgcof, Drhs, ubarclm - ubar(krhs) into rhs_ubar / rhs_vbar, predictor and
 *                corrector, before the coupling with rufrc (step2d_LF_AM3.h:1818-1845)
 *   every RadNud edge of a variable whose switch is on: obc_out = the coefficient at the edge (tracers: at the
 *                boundary point, t3dbc_im.F:119-126, :254, :388, :522; momentum: the mean of the two rho-points around
 *                the velocity point, u3dbc_im.F:113, v3dbc_im.F:113, u2dbc_im.F:149-158, v2dbc_im.F:151-158 and the
 *                other edges' blocks), obc_in = obcfac * obc_out, instead of roms_params_t.obc_out / obc_in; also in
 *                pre_step3d (pre_step3d.F:1126-1135) and ini_fields (ini_fields.F:602-633).  zetabc.F has no such
 *                branch.
 * Call it after roms_hip_set_bounds and roms_hip_set_params, and again whenever set_data has moved the climatology:
 * on a later call with the same switches a NULL array means "keep the copy you have".  A set switch whose arrays were
 * never given, obcfac < 0 and a call before bounds / params are refused.  All switches zero releases everything.
 * roms_hip_set_bounds drops the copies (new extents). */
int roms_hip_set_clima(int LnudgeM2CLM, const double *M2nudgcof, const double *ubarclm, const double *vbarclm,
                       int LnudgeM3CLM, const double *M3nudgcof, const double *uclm, const double *vclm,
                       const int *LnudgeTCLM, const double *Tnudgcof, const double *tclm, double obcfac);
/* One of the eight device copies ("M2nudgcof", "ubarclm", ..., "tclm") back to host memory, ordered after the kernels
 * issued; n_doubles is checked.  For a host that writes out the climatology roms_hip_set_data interpolates, and for tests. */
int roms_hip_get_clima(const char *name, double *host, long n_doubles);
/* Time-averaged fields (AVERAGES): set_avg(ng,tile), ROMS/Nonlinear/set_avg.F:28, called after set_zeta
 * (main3d.F:493-495).  The averages are device arrays of the library, one per selected line of roms_avg.def, with the
 * tile's extents (LBi:UBi, LBj:UBj [, N | 0:N]) and zero wherever the reference's loops do not reach.
 *
 * roms_hip_set_averages hands over the window nAVG, its first step ntsAVG, ntstart and nrrec (mod_scalars.F) and the
 * selection: Aout[AVG_COUNT] (0 / 1 per id of enum roms_avg_id; the entries of the per-tracer averages and of the
 * counters are not looked at) and AoutT[ROMS_AVG_NTKINDS][NT], row-major with rows of the tile's NT, the rows in the
 * order of the per-tracer lines of roms_avg.def (avgt, avgTT, avgUT, avgVT, avgHuonT, avgHvomT); NULL = none.  It
 * allocates the selected arrays zero-filled, with wet_dry also the four counters pmask_avg ... vmask_avg; an earlier
 * selection is released first.  nAVG = 0 releases everything; roms_hip_set_bounds drops the arrays.  Refused, leaving
 * the library as it was: a call before bounds / params, nAVG < 0, a selected average that is not built (named in the
 * error text), a selected average whose source field is not registered.
 *
 * roms_hip_set_avg reads s->iic, kstp, nrhs: one launch initialises, accumulates or accumulates-and-scales every
 * selected average (set_avg.F:237-240, :1264, :2298-2301); after a close the ghost points are filled where the
 * reference fills them (a periodic direction).  With wet_dry the blocks multiply by the *_full mask of their grid type,
 * the counters count the wet steps, the close divides by max(1, count) and then clamps the counters to 1
 * (set_masks.F:466-512).  Without a selection, or with nAVG = 0, it returns 0 and does nothing.
 *
 * roms_hip_get_average copies one average (itrc = 1-based tracer of a per-tracer average, otherwise ignored) or one
 * counter to host memory, ordered after the kernels issued; n_doubles is checked against the array.  The host's
 * wrt_avg calls it on the steps where the window closes.  roms_hip_average_device_ptr: the device array, NULL if none. */
#define ROMS_AVG_NTKINDS 6
enum roms_avg_id {
#define ROMS_AVG(name, aout, grid, shape, mask, range, expr, srcA, srcB, plane) AVG_##name,
#define ROMS_AVG_NOT_BUILT(name, aout, why) AVG_##name,
#define ROMS_AVG_COUNTER(name, grid) AVG_##name,
#include "roms_avg.def"
#undef ROMS_AVG
#undef ROMS_AVG_NOT_BUILT
#undef ROMS_AVG_COUNTER
  AVG_COUNT
};
int roms_hip_set_averages(int nAVG, int ntsAVG, int ntstart, int nrrec, const int *Aout, const int *AoutT);
int roms_hip_set_avg(const roms_step_idx_t *s);
int roms_hip_get_average(int avg_id, int itrc, double *host, long n_doubles);
double *roms_hip_average_device_ptr(int avg_id, int itrc);
/* Host-only (no GPU): what set_avg does at time step iic, as a sum of 1 = initialise (set_avg.F:237-240), 2 = accumulate
 * (:1264), 4 = scale, "close" (:2298-2301), 8 = clamp the WET_DRY counters (set_masks.F:466-468: no nAVG = 1 branch);
 * 0 with nAVG = 0.  The one statement of the schedule: roms_hip_set_avg asks it, the tests compare it with a table. */
int roms_hip_avg_phase(int iic, int nAVG, int ntsAVG, int ntstart, int nrrec);
/* Tracer budget diagnostics (DIAGNOSTICS_TS): set_diags(ng,tile), ROMS/Utility/set_diags.F:28, called after set_zeta
 * and before set_avg (main3d.F:490-492), and the DiaTwrk statements of pre_step3d.F:894-904, t3dmix2_s.h:293-296 and
 * step3d_t.F:868-871, :1199-1205, :1417-1427, :1475-1500, :1598-1611, which roms_hip_pre_step3d, roms_hip_t3dmix2 and
 * roms_hip_step3d_t carry out while the diagnostics are on.  The terms are those of roms_dia.def; the library owns
 * DiaTwrk and DiaTrc (LBi:UBi, LBj:UBj, N, NT, NDT), avgzeta (LBi:UBi, LBj:UBj) and with wet_dry rmask_dia.  The momentum
 * half, DIAGNOSTICS_UV, is not built and has no switch here.
 *
 * roms_hip_set_diagnostics hands over the window nDIA, its first step ntsDIA, ntstart and nrrec (mod_scalars.F) and
 * allocates the arrays zero-filled (mod_diags.F), NDT = 6 without ts_dif2 and 9 with it; an earlier set is released
 * first.  nDIA = 0 releases everything and the step runs the kernels it runs without diagnostics; roms_hip_set_bounds
 * drops the arrays.  Refused by name, leaving the library as it was: a call before bounds / params, nDIA < 0, MPDATA or
 * HSIMT tracers, ts_dif4, rotated mixing (ts_dif2 with mix_geo_ts or mix_iso_ts: iTsdif), point sources.  The entries
 * above refuse the same when the parameters change afterwards (a change of ts_dif2 asks for a new call).
 *
 * roms_hip_set_diags reads s->iic and s->kstp: one launch initialises or accumulates DiaTrc, avgzeta (from
 * zeta(:,:,kstp)) and the counter over IstrR:IendR, JstrR:JendR (set_diags.F:121-124, :244; the schedule is the
 * initialise / accumulate part of roms_hip_avg_phase with nDIA, ntsDIA), with wet_dry weighted by rmask_full.  The
 * scaling by the window length at output time (:374-1010, with wrt_diags) stays with the host.  With nDIA = 0 it
 * returns 0 and does nothing.  Timer name: "set_diags".
 *
 * roms_hip_get_diagnostic copies the plane (LBi:UBi, LBj:UBj, N) of term dia_id and tracer itrc (1-based) to host
 * memory, DiaTwrk with accumulated = 0 and DiaTrc with accumulated = 1; DIA_avgzeta and DIA_rmask_dia return those 2-D
 * arrays (itrc, accumulated not looked at).  A term that is not present (the iT?dif without ts_dif2, iTsdif) is refused.
 * roms_hip_dia_index (host-only, no GPU): the reference's idiag (1-based, mod_scalars.F:4027-4043) of a term for a
 * build with / without horizontal diffusion and rotated mixing, 0 where the term is not present; dia_id = DIA_COUNT
 * returns NDT. */
enum roms_dia_group { DIA_ALWAYS = 0, DIA_HDIF = 1, DIA_ROT = 2 };
enum roms_dia_id {
#define ROMS_DIA(name, group, what) DIA_##name,
#define ROMS_DIA_RESERVED(name, what)
#include "roms_dia.def"
#undef ROMS_DIA
#undef ROMS_DIA_RESERVED
  DIA_COUNT,
  DIA_RESERVED_BASE = DIA_COUNT,
#define ROMS_DIA(name, group, what)
#define ROMS_DIA_RESERVED(name, what) DIA_##name,
#include "roms_dia.def"
#undef ROMS_DIA
#undef ROMS_DIA_RESERVED
  DIA_END
};
int roms_hip_set_diagnostics(int nDIA, int ntsDIA, int ntstart, int nrrec);
int roms_hip_set_diags(const roms_step_idx_t *s);
int roms_hip_get_diagnostic(int dia_id, int itrc, int accumulated, double *host, long n_doubles);
int roms_hip_dia_index(int dia_id, int hdif, int rotated);
/* Lagrangian floats (FLOATS): step_floats(ng, Lstr, Lend), ROMS/Nonlinear/step_floats.F:80-1053, with interp_floats
 * (ROMS/Nonlinear/interp_floats.F:56-541), the block at the end of the step (main3d.F:873-906).  Built for SOLVE3D and
 * FLOATS with or without MASKING; not built: FLOAT_VWALK, FLOAT_STICKY, FLOAT_BIOLOGY / FLOAT_OYSTER, the 2-D branch,
 * N-S periodic grids.  NFT = 4 time levels 0:NFT, NFV = NT + 10 variables, the indices of mod_floats.F:80-90.
 * Precondition, as in the reference: a float moves less than one cell per step, so that its owner reads at most two
 * ghost points.
 *
 * roms_hip_set_floats hands DRIFTER(ng) over once: Ftype(Nfloats) (1 = flt_Lagran, 2 = flt_Isobar, 3 = flt_Geopot),
 * Tinfo(0:izrhs,Nfloats) in Fortran order, Fz0(Nfloats), and the two coordinate arrays iflon / iflat are interpolated
 * from (lonr, latr if spherical, else xr, yr; extents LBi:UBi,LBj:UBj).  All are copied.  track and bounded are
 * allocated zero-filled (mod_floats.F:219-246); an earlier set is released first.  Nfloats = 0 releases everything;
 * roms_hip_set_bounds drops them.  Refused, leaving the library as it was: a call before bounds / params, an Ftype
 * outside 1..3, N-S periodic bounds.
 *
 * roms_hip_floats_put / roms_hip_floats_get copy track(NFV,0:NFT,Nfloats) and bounded(Nfloats) (0 / 1) in the host's
 * element order (restart; get before wrt_floats), ordered after the kernels issued; n_track = NFV*(NFT+1)*Nfloats and
 * n_bounded = Nfloats are checked.
 *
 * roms_hip_step_floats: nfl = {nfm3, nfm2, nfm1, nf, nfp1} (a permutation of 0..4, refused otherwise), time = time(ng)
 * before main3d.F:914 advances it; reads s->nnew.  The caller rotates the five indices afterwards (main3d.F:899-903).
 * Ownership (:185-207), Milne predictor (:238-346), slopes (:353-389), Hamming corrector (:465-579), status
 * (:585-691), release (:698-748), slopes and outputs at the corrected position (:755-960), reflection (:1009-1021), and
 * the collection over the tiles (mp_collect, :1030-1049; with E-W periodicity on several tile columns also :604-627)
 * over the active transport.  On one tile nothing is collected; the ownership switch is applied all the same (rank 0
 * is the master).  Without floats it returns 0 and does nothing.  Timer name: "step_floats". */
int roms_hip_set_floats(int Nfloats, const int *Ftype, const double *Tinfo, const double *Fz0,
                        const double *xcoord, const double *ycoord);
int roms_hip_floats_put(const double *track, long n_track, const int *bounded, long n_bounded);
int roms_hip_floats_get(double *track, long n_track, int *bounded, long n_bounded);
int roms_hip_step_floats(const roms_step_idx_t *s, double time, const int nfl[5]);
/* Tidal forcing of the open boundaries (SSH_TIDES, UV_TIDES): set_tides(ng,tile), ROMS/Nonlinear/set_tides.F:28, called
 * after set_vbc (main3d.F:395-397).  Built with or without MASKING, RAMP_TIDES, ADD_FSOBC, ADD_M2OBC; not built:
 * AVERAGES_DETIDE, TIDE_GENERATING_FORCES, the CLIMA(ng)%ssh / ubarclm / vbarclm additions of the two ADD options, N-S
 * periodic grids.
 *
 * roms_hip_set_tides hands TIDES(ng) over: NTC constituents of MTC planes, Tperiod[MTC] (s; a constituent with
 * Tperiod <= 0 is skipped), SSH_Tamp, SSH_Tphase (both, or both NULL: SSH_TIDES), UV_Tangle, UV_Tphase, UV_Tmajor,
 * UV_Tminor (all four, or all NULL: UV_TIDES), each (LBi:UBi, LBj:UBj, MTC) in the host's layout with the ghost points
 * filled (one ghost point beside the tile is read; no exchange is made), angles and phases in radians; angler
 * (LBi:UBi, LBj:UBj; NULL = zero); tide_start (days), ramp_tides (0 / 1: RAMP_TIDES) with dstart (days); add_fsobc with
 * zeta_base and add_m2obc with ubar_base, vbar_base: the sub-tidal boundary data (LBi:UBi, LBj:UBj, the point
 * convention of zeta_bry / ubar_bry / vbar_bry).  The library keeps device copies of the bases and writes base + tide
 * every step -- never += on its own output, which the reference gets from set_data refreshing BOUNDARY(ng) first; a
 * later call with a NULL base keeps the copy.  Only the two lines of rho-points beside each edge are kept on the
 * device (edge-major strips, gathered one constituent plane at a time), with the land/sea masks of those lines as the
 * device holds them at this call: call it again after uploading other masks or changing roms_params_t.masking.
 * Refused, leaving the library as it was: a call before bounds / params; NTC < 0, NTC > MTC, NTC > 32; one array of the
 * pair or of the quadruple missing; NTC > 0 with neither group; an ADD option without its group or its base; add_m2obc
 * while LnudgeM2CLM is on (set_tides.F:476-508 then moves ubarclm / vbarclm as well); masking = 1 before the masks are
 * registered; N-S periodic bounds.  NTC = 0 with all arrays NULL releases everything; roms_hip_set_bounds drops the
 * strips.  With SSH_TIDES alone the Flather and Shchepetkin conditions of the normal barotropic velocity take the
 * reduced-physics boundary value instead of ubar_bry / vbar_bry (u2dbc_im.F:219-255, :291-327, :567-603, :639-675 and the
 * four blocks of v2dbc_im.F); the captured LOOP_2D graphs are dropped when that switch changes.
 *
 * roms_hip_tides: time = time(ng) at the call, before main3d.F:914 advances it.  One launch evaluates the harmonics
 * and writes zeta_bry (a side's free surface, ubar or vbar acquires boundary data: Cla, Fla, Shc, RadNud; Fla / Shc on
 * ubar or vbar count for the free surface, inp_decode.F:1621-1655), ubar_bry and vbar_bry (a side's ubar and vbar both
 * acquire) on the tiles of a physical, non-periodic edge, over the reference's ranges -- but for the four corner
 * rho-points of zeta_bry, which no condition reads (k_set_tides.hip).  Without tides it returns 0 and does nothing.
 * Timer name: "set_tides". */
int roms_hip_set_tides(int NTC, int MTC, const double *Tperiod, const double *SSH_Tamp, const double *SSH_Tphase,
                       const double *UV_Tangle, const double *UV_Tphase, const double *UV_Tmajor, const double *UV_Tminor,
                       const double *angler, double tide_start, int ramp_tides, double dstart,
                       int add_fsobc, const double *zeta_base, int add_m2obc, const double *ubar_base,
                       const double *vbar_base);
int roms_hip_tides(double time);
/* Forcing, boundary and climatology snapshots: set_data(ng,tile), ROMS/Nonlinear/set_data.F:20-1390, called at
 * main3d.F:222 before ini_fields, the surface physics and set_tides.  The calls of set_2dfld_tile (ROMS/Utility/set_2dfld.F:21),
 * set_3dfld_tile (set_3dfld.F:21) and set_ngfld (set_ngfld.F:21) for the targets of include/roms_data.def: the host hands
 * each time record over once, when get_data has read it, and every step one launch interpolates all of them.
 *
 * roms_hip_set_data_record: one record of target (enum roms_data_id).  index = itrc (1-based) of stflux / btflux /
 * t_bry, the compact index ic (1-based, step3d_t.F:1551-1560) of tclm, not looked at otherwise; side = enum
 * roms_lbc_side of an open-boundary target, not looked at otherwise.  slot in {1, 2} = the reference's Tindex =
 * Iinfo(8,ifield,ng) after the read: the slot of the latest call is it2, the other one it1 = 3 - Tindex
 * (set_2dfld.F:91-92).  Tintrp = Tintrp(slot,ifield,ng) in seconds, onerec = Linfo(3,ifield,ng).  rec has the extents the
 * table gives for the target's shape (gridded: the host's Finp(:,:,slot) with the tile's LBi:UBi, LBj:UBj [, N]; an edge:
 * the slice LBj:UBj or LBi:UBi [, N] of zeta_west(:), u_south(:,N), t_north(:,N) ..., Fortran order); n_doubles is checked.
 * The record is copied to a device array of the library on the library's stream, behind the kernels that read the slot's
 * old contents; the host buffer is free on return; nothing but that stream is waited for.  An edge record is kept as an
 * edge-major strip, never as a tile-sized array.  A record for a side that is not a physical (non-periodic) edge of this
 * tile returns 0 and keeps nothing.  A climatology target whose device copy does not exist (its switch is off) is
 * refused: hand the arrays over with roms_hip_set_clima first.
 * roms_hip_set_data_point: the same for point data, Linfo(1,ifield,ng) = .FALSE.: value = Fpoint(slot,ifield,ng); the
 * targets of set_2dfld only.  The result is the uniform field of set_2dfld.F:127-133.
 *
 * roms_hip_set_data(time, dt, &synchro): time = time(ng), dt = dt(ng).  For every target with records the host evaluates
 * set_2dfld.F:90-94, :116-120 in double (roms_hip_set_data_factors); *synchro is set to 1 where time + dt >
 * Tintrp(it2) for any target (:139-141) and to 0 otherwise.  All or nothing: every target is checked before anything is
 * launched, and if one fails the call returns non-zero, the message holds the target's name, "exceeds ending value" and
 * the two record times (set_2dfld.F:156-162), and no target is written.  Then ONE launch writes
 * Fout = fac1*Finp(it1) + fac2*Finp(it2) (onerec: Finp(Tindex)) for all targets: gridded ones on IstrR:IendR,
 * JstrR:JendR, followed by the periodic images and the tile exchange of set_2dfld.F:170-201 / set_3dfld.F:183-219 in one
 * packed exchange; edge ones on the row or column of the *_bry field where roms_fields.def puts the edge value, over the
 * points of the allocated extent inside the reference's range (0 or 1 : Lm+1 / Mm+1).  With add_fsobc / add_m2obc tides
 * the results for zeta_bry / ubar_bry, vbar_bry go into the tides' zeta_base / ubar_base, vbar_base copies, so that
 * roms_hip_set_data followed by roms_hip_tides gives base + tide, as the reference's order does.  With wet_dry the
 * interpolated zeta_bry is clipped to Dcrit - h on IstrR:IendR / JstrR:JendR of the edge in the same pass (:928-1003).
 * A target with no records is not touched: roms_hip_sync_to_device and roms_hip_set_clima keep working for it, and a
 * library in which no record was ever set behaves as before (the call returns 0 and launches nothing).
 * Refused, leaving the library as it was: a call before bounds / params; an unknown target, index or side; a wrong length;
 * slot outside 1..2; at roms_hip_set_data a target with a slot never filled (unless onerec).  roms_hip_set_bounds drops
 * all records.  Timer name: "set_data".
 *
 * roms_hip_set_data_factors (host only, no GPU): the statement of set_2dfld.F:90-120 for Tintrp(1) = T1, Tintrp(2) = T2:
 * fac1 (of it1 = 3 - Tindex), fac2 (of it2 = Tindex) and *synchro (set to 1 where :139 holds, left alone otherwise);
 * onerec gives fac1 = 0, fac2 = 1.  Non-zero where the reference takes its error branch (:145).
 *
 * Not built, see roms_data.def: the CURVGRID rotation of point or coarse winds and stresses, DIURNAL_SRFLUX, the source
 * table (roms_hip_set_sources), wave data, the 4D-Var blocks, CLIMA%ssh.  A host with one of those keeps interpolating
 * that field itself and uploads it (roms_hip_sync_to_device). */
enum roms_data_shape { DS_2D = 0, DS_N, DS_2DT, DS_NC, DS_E, DS_EN, DS_ENT };
enum roms_data_dest { DD_FIELD = 0, DD_CLIMA, DD_BRY };
enum roms_data_id {
#define ROMS_DATA(name, routine, grid, shape, dest) DATA_##name,
#include "roms_data.def"
#undef ROMS_DATA
  DATA_COUNT
};
int roms_hip_set_data_record(int target, int index, int side, int slot, double Tintrp, int onerec,
                             const double *rec, long n_doubles);
int roms_hip_set_data_point(int target, int index, int slot, double Tintrp, int onerec, double value);
int roms_hip_set_data(double time, double dt, int *synchro);
int roms_hip_set_data_factors(double time, double dt, double T1, double T2, int Tindex, int onerec,
                              double *fac1, double *fac2, int *synchro);
/* wvelocity(ng,tile,nstp)         ROMS/Nonlinear/wvelocity.F:27     (main3d.F:475; writes wvel) */
int roms_hip_wvelocity(const roms_step_idx_t *s);
/* diag(ng,tile)                    ROMS/Nonlinear/diag.F:31          (main3d.F:314), the tile-local part
 * diag.F:190-290 on time level nstp: out12 = { my_volume, my_avgke, my_avgpe, my_maxspeed, my_maxrho,
 * my_max_C, my_max_Cu, my_max_Cv, my_max_Cw, my_max_Ci, my_max_Cj, my_max_Ck } (host memory; the call
 * returns when they are there).  The reduction over tiles -- mp_reduce SUM/SUM/SUM/MAX/MAX and
 * mp_reduce2 MAXLOC, diag.F:398-420 -- and the printing stay with the caller. */
int roms_hip_diag(const roms_step_idx_t *s, double *out12);

/* The whole barotropic loop LOOP_2D of main3d.F:592-700 in one call
 * (predictor/corrector sequencing done inside: 2*nfast+1 launches queued on the library's
 * stream without returning to the host).  indx1 is mod_stepping's indx1(ng), updated on return.
 * Equal, bit for bit, to the same 2*nfast+1 roms_hip_step2d calls; the two may be mixed from step to step.
 * On one tile the launches are captured once per (indx1, nstp, nnew, start-up phase) and replayed.  Between steps a
 * caller may, at the stated cost:
 *   - hand over new values on the same source faces (roms_hip_set_sources), new climatology arrays under the same
 *     switches and obcfac (roms_hip_set_clima), upload any field that is not a grid metric, switch averages or
 *     floats: nothing is recaptured;
 *   - call roms_hip_set_params, register a field again, change the source faces or their number (0 included), the
 *     climatology switches or obcfac, roms_hip_graph_exchanges: the graphs are dropped and captured again (one
 *     eager-cost loop per key, up to four);
 *   - upload a grid-metric array, h, visc2_r or visc2_p: the row table is examined again at the next barotropic
 *     call (one small kernel and one synchronisation) and the graphs are captured again;
 *   - roms_hip_set_bounds: everything, see there.
 * The results are those of a fresh context started from the same fields (tests/test_gpu_context_reuse.py). */
int roms_hip_step2d_loop(roms_step_idx_t *s, int *indx1);

/* Several tiles over RCCL: replay LOOP_2D as ONE hipGraph that contains the compute launches, the pack / unpack
 * launches and the ncclSend / ncclRecv groups of its 2*nfast+1 calls (RCCL enqueues its kernels on the capturing
 * stream).  Every rank of the communicator must switch it on before its first roms_hip_step2d_loop, since all of
 * them then capture once and replay the same sequence.  Off by default: on this stack the replay shortens the loop's
 * device time (BENCHMARK1 tile, loopback: 1.85 -> 1.65 ms) but lengthens the step's wall time (3.05 -> 3.64 ms).  If
 * the stack refuses the capture the loop keeps running eagerly.  state: 0 = eager, 1 = graph in use, -1 = capture was
 * tried and refused.  (the reference's loop is step2d_LF_AM3.h:509-590 per call.) */
int roms_hip_graph_exchanges(int on);
int roms_hip_graph_exchanges_state(void);

/* mp_exchange2d/3d/4d (ROMS/Utility/mp_exchange.F:290/1413/2753) together
 * with the periodic exchange_*_tile (exchange_2d.F:229, exchange_3d.F:259) on
 * whole registered fields; level = 1-based trailing index (time level or
 * tracer) or 0 for all.  Exported for tests. */
int roms_hip_exchange(int field_id, int level);

/* Second halo transport: a host relay.  When roms_hip_init got no RCCL id (NULL) on a
 * multi-tile run, every exchange packs its messages on the device (one per neighbour tile: W, E, S, N
 * and the four diagonal ones, as far as they exist), copies them to pinned host memory and calls `fn`,
 * which must deliver send[m].buf (count doubles) to rank send[m].peer with message tag send[m].tag and
 * fill recv[m].buf from rank recv[m].peer, tag recv[m].tag -- e.g. with the MPI_Isend / MPI_Irecv /
 * MPI_Waitall the reference's mp_exchange2d (ROMS/Utility/mp_exchange.F:290-560) already uses.  Two
 * messages between the same pair of ranks differ in their tag.  Return 0 on success.
 * The RCCL transport is the fast one; the relay exists for hosts that own the
 * interconnect and for rehearsing N tiles on fewer GPUs. */
typedef struct { int peer; int tag; long count; double *buf; } roms_halo_msg_t;
typedef int (*roms_halo_relay_fn)(void *user, int nsend, const roms_halo_msg_t *send,
                                  int nrecv, const roms_halo_msg_t *recv);
int roms_hip_set_halo_relay(roms_halo_relay_fn fn, void *user);
/* Host-only (no GPU): the messages tile `rank` exchanges per halo update for the bounds *b:
 * out = nsend, nrecv, then (peer, tag, i0, wi, j0, wj) per message, sends first; at most 8 + 8 messages
 * (98 ints).  Exported for the CPU tests, which play a whole 4x2 exchange with it. */
int roms_hip_halo_plan(const roms_bounds_t *b, int rank, int *out);

/* Timing helper: average device milliseconds of the last call of each entry
 * measured with hipEvents on the library's stream (bench.py roofline). */
int roms_hip_timing_enable(int on);
double roms_hip_timing_last_ms(const char *entry);

/* Profiling aid (no reference counterpart): one streaming copy of n_doubles
 * from 3-D scratch array 0 to scratch array 1 in the library's access pattern
 * (one double per lane, i-fastest).  A known byte count -- 8*n read, 8*n
 * written -- against which rocprofv3's FETCH_SIZE / WRITE_SIZE counters are
 * calibrated for this pattern.  n_doubles <= nij*(N+1). */
int roms_hip_calib_stream(long n_doubles);

/* Debugging aid (no reference counterpart): every device mirror and scratch array carries a guard band of
 * four rows on either side, filled with one NaN bit pattern.  Returns 0 when every band is intact, an
 * error naming the array otherwise (a kernel stored outside LBi:UBi,LBj:UBj at the first or last plane).
 * Reads in the band are harmless by construction and deliver NaN. */
int roms_hip_check_guards(void);
/* The arrays roms_hip_check_guards looks at -- every live guarded array, in allocation order: returns their number
 * and, where buf is not NULL, writes their names into buf[cap] as one C string, a line each: NAME, or NAME[q] for
 * the indexed scratch arrays (a buffer too small cuts the list).  -1 without roms_hip_init. */
long roms_hip_guarded_arrays(char *buf, long cap);

#ifdef __cplusplus
}
#endif
#endif /* ROMS_HIP_H */
