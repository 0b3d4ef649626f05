/*
 * ntm_mpc.h — C-ABI of the MI355X-native batched LPV-MPC hot path.
 *
 * Drop-in boundary for the receding-horizon loop of the MATLAB reference
 * IsaacSavona/MPC-NTM-Control (NTM_MPC_Sim.m:93-131).  The reference has no
 * FFI of its own: its hot path is a set of MATLAB functions resolved by name
 * (rho1.m, rho2.m, rho3.m, A.m, B.m, Rho_to_PhiGammaLambda.m, getWLc.m and
 * MathWorks quadprog).  Function-handle arguments cannot cross a C ABI, so the
 * boundary sits at the time-step level (one MEX call replaces lines 94-130 for
 * a whole batch of scenarios) plus one entry point per reference function for
 * per-function parity.  See INTEGRATION.md for the MEX / ctypes bindings.
 *
 * Conventions
 *  - fp64 everywhere; all per-scenario matrices are MATLAB column-major.
 *  - Batched arrays are scenario-major: a per-scenario record of E elements
 *    is contiguous, element e of scenario s at [s*E + e].  In MATLAB this is
 *    an E-by-B array with one column per scenario (x0 is 2-by-B, U is N-by-B,
 *    rho is 3N-by-B), and a contiguous range of scenarios (one GPU's shard) is
 *    a contiguous block of memory.  The time histories of ntm_mpc_run are
 *    E-by-k_sim-by-B.  (ABI v2 was scenario-minor, [e*B + s].)
 *    Exception: the optional instrumentation counters (ntm_ctx_set_stats).
 *  - Host-pointer entry points (no suffix) stage through the device and are
 *    synchronous.  *_device entry points take device pointers and a
 *    hipStream_t (as void*), enqueue only, and never synchronise.
 *  - Return value: NTM_OK (0) or a negative NTM_E_* code; the message is in
 *    ntm_last_error(ctx).  Per-scenario solver outcomes are NOT errors: they
 *    are reported in exitflag[] with quadprog's codes (NTM_MPC_Sim.m:98-103).
 *  - Caller owns every array; the library never retains a pointer past the
 *    call.  One call at a time per ntm_ctx.
 */
#ifndef NTM_MPC_H
#define NTM_MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTM_MPC_ABI_VERSION 7   /* v7: ntm_estimator, ntm_mpc_step_est / run_est, ntm_meas_sample (additive);
                                   still 7: ntm_mpc_run_from / run_est_from (additive, NTM_MPC_HAS_RUN_FROM);
                                   still 7: ntm_delay, ntm_mpc_step_dly / run_dly / run_dly_from (additive,
                                   NTM_MPC_HAS_INPUT_DELAY);
                                   v6: ntm_observer, ntm_mpc_step_obs / run_obs (additive);
                                   v5: ntm_config.Ru (input weight); v4: ntm_scenario_gen */
#define NTM_MAX_N 64
/* ntm_mpc_run_from* / ntm_mpc_run_est_from* exist (added without an ABI bump) */
#define NTM_MPC_HAS_RUN_FROM 1
/* ntm_delay and ntm_mpc_step_dly* / ntm_mpc_run_dly* / ntm_mpc_run_dly_from* exist (added
 * without an ABI bump) */
#define NTM_MPC_HAS_INPUT_DELAY 1
#define NTM_MAX_DELAY 8         /* longest actuator dead time, in sampling periods */

/* Physics constants, NTM_MPC_Sim.m:5-22 (same names and units). */
typedef struct {
    double j_BS, w_dep, w_marg, w_sat, tau_r, rs, a, eta_CD, tau_E0, tau_E,
           mu0, Lq, B_pol, m, Cw, tau_A0, tau_w, omega0;
} ntm_physics;

/* Constraint modes. */
enum { NTM_MODE_NONE = 0,   /* unconstrained LQ (BASELINE config 1)       */
       NTM_MODE_BOX = 1,    /* u in [umin, umax] only (config 2)          */
       NTM_MODE_FULL = 2,   /* full getWLc.m polyhedron, m = 6N+4 (cfg 3) */
       NTM_MODE_FULL_DU = 3 }; /* getWLc rows + input-rate rows
                                *   |U_i - U_{i-1}| <= du_max, i = 1..N-1,
                                * m = 8N+2 (BASELINE config 5; an extension
                                * of getWLc.m's row structure, not in the
                                * reference) */

/* Literal-reference switches; 0 = canonical semantics. */
enum { NTM_LITERAL_PHI_RIGHTMUL = 1 << 0,  /* D4  Rho_to_PhiGammaLambda.m:21 */
       NTM_LITERAL_GAMMA_INDEX = 1 << 1,   /* D6  Rho_to_PhiGammaLambda.m:32 */
       NTM_LITERAL_PLANT_NO_C = 1 << 2,    /* D13 NTM_MPC_Sim.m:130          */
       NTM_RHO1_SQUARED = 1 << 3 };        /* D18 rhos.m:18                  */

/* Controller configuration, NTM_MPC_Sim.m:30-60, 80-88. */
typedef struct {
    int32_t N;          /* :30 prediction horizon, 1..NTM_MAX_N            */
    int32_t i_sim;      /* :81 max LPV scheduling iterations               */
    int32_t mode;       /* NTM_MODE_*                                      */
    int32_t flags;      /* NTM_LITERAL_* / NTM_RHO1_SQUARED                */
    double Ts;          /* :31                                             */
    double xmin[2];     /* :44                                             */
    double xmax[2];     /* :45                                             */
    double umin, umax;  /* :49-50                                          */
    double Q[4];        /* :59 state weight, row-major 2x2, symmetric PSD  */
    double r[2];        /* :60 reference state                             */
    double epsilon;     /* :87 convergence threshold on sum|U - Uold|      */
    double du_max;      /* NTM_MODE_FULL_DU only: input-rate bound (W/step) */
    double Ru;          /* input weight R_u >= 0: the cost of
                         * NTM_MPC_Sim.m:71-73,120 becomes G = 2 Gamma' Om Gamma
                         * + 2 Ru I (F unchanged).  The reference has none: 0,
                         * its default, is the reference's cost (ABI v5).  A
                         * non-zero Ru runs on the generic (runtime-N) kernels. */
} ntm_config;

/* Return codes. */
enum { NTM_OK = 0, NTM_E_INVALID = -1, NTM_E_DEVICE = -2, NTM_E_NOMEM = -3,
       NTM_E_UNSUPPORTED = -4 };

/* Per-scenario QP exit flags (quadprog convention, NTM_MPC_Sim.m:98-103). */
enum { NTM_EXIT_OPTIMAL = 1, NTM_EXIT_MAXITER = 0, NTM_EXIT_INFEASIBLE = -2,
       NTM_EXIT_NONFINITE = -7 };

/* Defaults = the reference's hard-coded literals (NTM_MPC_Sim.m:5-88). */
void ntm_physics_default(ntm_physics* p);
void ntm_config_default(ntm_config* c, int32_t N);
int32_t ntm_abi_version(void);

typedef struct ntm_ctx ntm_ctx;
int ntm_ctx_create(ntm_ctx** out, int32_t device);
void ntm_ctx_destroy(ntm_ctx* ctx);
const char* ntm_last_error(const ntm_ctx* ctx);
/* Optional instrumentation: device array of NTM_STATS_ROWS*B int32 (SoA, row
 * k of scenario s at [k*B + s]) that subsequent step/run launches ACCUMULATE
 * into: 0 QP solves, 1 Goldfarb-Idnani iterations, 2 final active rows,
 * 3 general (state) active rows, 4 warm-start candidate verifications,
 * 5 full Goldfarb-Idnani solves.  NULL disables. */
#define NTM_STATS_ROWS 6
int ntm_ctx_set_stats(ntm_ctx* ctx, int32_t* dev_stats);
/* Workspace layout of the N = 20 step/run kernels by batch size: batches of at
 * most max_scenarios run on the all-LDS build (2 waves per SIMD), larger ones on
 * the far-workspace build (4 waves per SIMD, GI factors in a per-scenario HBM
 * block).  Default (and max_scenarios < 0): 8 x the device's compute units, the
 * measured crossover (2048 on an MI355X); 0 = always the far build.  Results of
 * the two builds agree to the parity tolerances, not bit for bit; within one
 * build a scenario's results do not depend on the batch around it. */
int ntm_ctx_set_small_batch(ntm_ctx* ctx, int64_t max_scenarios);
/* Among the all-LDS N = 20 batches, those of at most max_scenarios run with a
 * one-wave-per-SIMD register budget (round 6): default (and < 0) 4 x the compute
 * units (1024 on an MI355X: one wave per SIMD), 0 = never.  Bit-identical
 * results to the two-wave budget; only the speed differs. */
int ntm_ctx_set_one_wave_batch(ntm_ctx* ctx, int64_t max_scenarios);
/* The build a step/run launch of B scenarios with cfg takes on this context:
 * *build = 0 far workspace, 1 all-LDS, 2 all-LDS with the one-wave budget. */
int ntm_ctx_step_build(const ntm_ctx* ctx, const ntm_config* cfg, int64_t B, int32_t* build);
/* Which build a step/run launch of B scenarios at horizon N takes on this
 * context: *far = 1 for the far-workspace build, 0 for an all-LDS one. */
int ntm_ctx_step_layout(const ntm_ctx* ctx, int32_t N, int64_t B, int32_t* far);
/* The same for a full config, as the step/run launch of B scenarios would take it
 * (flags included: the literal D4/D6 switches run on the generic kernels) and
 * the launch shape of that kernel: lanes per scenario and the compile-time
 * horizon (0 = generic).  ntm_ctx_step_layout is this with the default config. */
int ntm_ctx_step_layout_cfg(const ntm_ctx* ctx, const ntm_config* cfg, int64_t B, int32_t* far, int32_t* lanes,
                            int32_t* horizon_template);
/* Diagnostic builds only: per-phase s_memtime cycle totals and counters (104 entries);
 * NTM_E_UNSUPPORTED in production builds. */
int ntm_debug_stamps(unsigned long long* out32, int reset);
/* Launch shape the step/run kernels use for horizon N: lanes per scenario
 * (16/32/64) and the compile-time horizon of the specialisation (0 = generic). */
int ntm_step_launch_info(int32_t N, int32_t* lanes, int32_t* horizon_template);

/* ---- time-step level: the drop-in for NTM_MPC_Sim.m:94-130 ------------ */
/* Initial LPV state for x0[2]: rho[3N] = repmat(rho(x0), 1, N)
 * (NTM_MPC_Sim.m:63-65) and U_old[N] = +Inf (the first convergence test never
 * passes, D14; the literal Uold = ones(...) at :86 is an implicit-expansion
 * defect). */
int ntm_mpc_init(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                 int64_t B, const double* x0, double* rho, double* U_old);
int ntm_mpc_init_device(ntm_ctx* ctx, const ntm_physics* phys,
                        const ntm_config* cfg, int64_t B, const double* x0,
                        double* rho, double* U_old, void* stream);
/* One MPC step for B scenarios.  In/out state per scenario:
 *   x_k[2], rho[3N] (3xN col-major: rows rho1,rho2,rho3; carried unshifted,
 *   D20), U_old[N] (persists across steps, D14; +inf on the first step).
 * Outputs: U[N] (last QP solve), x_pred[2(N+1)] (2x(N+1) rollout x_0..x_N),
 *   x_next[2] (plant step :130), exitflag (last QP), inner_iters (QP solves). */
int ntm_mpc_step(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                 int64_t B, const double* x_k, double* rho, double* U_old,
                 double* U, double* x_pred, double* x_next,
                 int32_t* exitflag, int32_t* inner_iters);
int ntm_mpc_step_device(ntm_ctx* ctx, const ntm_physics* phys,
                        const ntm_config* cfg, int64_t B, const double* x_k,
                        double* rho, double* U_old, double* U, double* x_pred,
                        double* x_next, int32_t* exitflag, int32_t* inner_iters,
                        void* stream);

/* Same, with an optional warm-start workspace carried from step to step:
 * active_ws[2(N+1)] int32 per scenario (in/out; initialise every entry to -1;
 * NULL = none) holds the active sets of the previous step's last two QPs.
 * They are tried first and taken only when the exact re-solve passes the KKT
 * certificate, so the result is the QP optimum either way;
 * entries that are not a valid active set are ignored.  ntm_mpc_run keeps
 * this state on chip by itself. */
int ntm_mpc_step_ws(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                    int64_t B, const double* x_k, double* rho, double* U_old,
                    double* U, double* x_pred, double* x_next,
                    int32_t* exitflag, int32_t* inner_iters, int32_t* active_ws);
int ntm_mpc_step_ws_device(ntm_ctx* ctx, const ntm_physics* phys,
                           const ntm_config* cfg, int64_t B, const double* x_k,
                           double* rho, double* U_old, double* U, double* x_pred,
                           double* x_next, int32_t* exitflag, int32_t* inner_iters,
                           int32_t* active_ws, void* stream);

/* Closed loop NTM_MPC_Sim.m:80-131 over k_sim steps, device-resident.
 * Per scenario: x0[2]; outputs xk[2(k_sim+1)] (2x(k_sim+1)), uk[k_sim],
 * Uk[N k_sim] (N x k_sim), wpred[(N+1) k_sim] ((N+1) x k_sim, predicted island
 * width per step), exitflag[k_sim], inner_iters[k_sim].  Any output pointer
 * may be NULL. */
int ntm_mpc_run(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                int64_t B, int32_t k_sim, const double* x0, double* xk,
                double* uk, double* Uk, double* wpred, int32_t* exitflag,
                int32_t* inner_iters);
int ntm_mpc_run_device(ntm_ctx* ctx, const ntm_physics* phys,
                       const ntm_config* cfg, int64_t B, int32_t k_sim,
                       const double* x0, double* xk, double* uk, double* Uk,
                       double* wpred, int32_t* exitflag, int32_t* inner_iters,
                       void* stream);

/* ntm_mpc_run from a carried state instead of x0: the same fused closed-loop kernels
 * with the controller state in and out, so a loop can be run in chunks (bounded
 * histories, a cfg / phys / generator that changes between chunks, checkpoint and
 * restart).  Per scenario, in/out and all required: x[2], rho[3N], U_old[N],
 * active_ws[2(N+1)] (the layouts of ntm_mpc_step_ws).  On return they hold the state
 * after step k_sim-1: x is the last plant state, the rest what a next call (or
 * ntm_mpc_step_ws) continues from.  Histories as ntm_mpc_run (any may be NULL); xk
 * column 0 is the input x.  k_sim = 0: nothing changes, xk column 0 is written.
 *  - The first call of a loop takes ntm_mpc_init's rho / U_old and active_ws all -1:
 *    exactly what ntm_mpc_run sets up inline.  k_sim steps in one call and the same
 *    steps split over several calls give the same bits, histories and state.
 *  - The generator's k0 is the caller's to advance between calls
 *    (ntm_ctx_set_scenarios): time index k0 + kk is used as in ntm_mpc_run.
 *  - cfg, phys and the generator may differ from call to call as long as N does not.
 *    Entries of active_ws that are not a valid active set under the new mode are
 *    ignored, as in ntm_mpc_step_ws; a caller who changes mode may reset them to -1.
 *  - Validation is ntm_mpc_run's; in addition a NULL state pointer is NTM_E_INVALID.
 *    x must not overlap xk.
 *  - The build is chosen as for ntm_mpc_run (ntm_ctx_step_build describes it), and the
 *    counters of ntm_ctx_set_stats accumulate across calls. */
int ntm_mpc_run_from(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                     int64_t B, int32_t k_sim, double* x, double* rho, double* U_old,
                     int32_t* active_ws, double* xk, double* uk, double* Uk,
                     double* wpred, int32_t* exitflag, int32_t* inner_iters);
int ntm_mpc_run_from_device(ntm_ctx* ctx, const ntm_physics* phys,
                            const ntm_config* cfg, int64_t B, int32_t k_sim, double* x,
                            double* rho, double* U_old, int32_t* active_ws, double* xk,
                            double* uk, double* Uk, double* wpred, int32_t* exitflag,
                            int32_t* inner_iters, void* stream);

/* ---- function level: one entry per reference function (device ptrs) --- */
/* rho1.m / rho2.m / rho3.m at x[2] -> rho[3]. */
int ntm_rho_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                   int64_t B, const double* x, double* rho, void* stream);
/* A.m / B.m at rho[3] -> A[4] (2x2 col-major), Bv[2] (2x1 column, D5). */
int ntm_AB_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                  int64_t B, const double* rho, double* A, double* Bv,
                  void* stream);
/* Rho_to_PhiGammaLambda.m: rho[3N] -> Phi[2N*2], Gamma[2N*N], Lambda[2N]. */
int ntm_lift_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                    int64_t B, const double* rho, double* Phi, double* Gamma,
                    double* Lambda, void* stream);
/* NTM_MPC_Sim.m:120-121: (rho, x_k) -> G[N*N], F[N]. */
int ntm_cost_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                    int64_t B, const double* rho, const double* x_k, double* G,
                    double* F, void* stream);
/* getWLc.m: rho -> W[m*2], L[m*N], c[m], m = 6N+4. */
int ntm_getwlc_device(ntm_ctx* ctx, const ntm_physics* phys,
                      const ntm_config* cfg, int64_t B, const double* rho,
                      double* W, double* L, double* c, void* stream);
/* quadprog stand-in (NTM_MPC_Sim.m:97): min 1/2 U'GU + F'U s.t. Lin U <= b,
 * G[N*N], F[N], Lin[m*N], b[m] per scenario -> U[N], exitflag. */
int ntm_qp_device(ntm_ctx* ctx, int64_t B, int32_t N, int32_t m,
                  const double* G, const double* F, const double* Lin,
                  const double* b, double* U, int32_t* exitflag,
                  int32_t* iters, void* stream);

/* Mixed precision (BASELINE config 5's "fp32 vs fp64" leg; NOT the fp64 product
 * path): the same QP as ntm_qp_device solved by Goldfarb-Idnani entirely in
 * fp32 on fp32-rounded data -> U32[N] (widened), then that active set re-solved
 * exactly in fp64 with the KKT certificate -> U[N]; if it does not certify, the
 * fp64 solve takes over.  info: bit 0 the fp32 active set certified, bit 1 fp64
 * fallback, bit 2 the fp32 solve itself was not optimal (U32 is then its last
 * iterate; 0 where the data leave fp32 no first one: non-finite or G not PD
 * after rounding, a violated constant row).  iters32: fp32 GI
 * iterations.  N <= 64, m <= 8N+4 rows within the 160 KiB LDS of one CU. */
int ntm_qp_mixed_device(ntm_ctx* ctx, int64_t B, int32_t N, int32_t m,
                        const double* G, const double* F, const double* Lin,
                        const double* b, double* U, double* U32, int32_t* exitflag,
                        int32_t* info, int32_t* iters32, void* stream);

/* ---- multipliers and the KKT audit ------------------------------------- */
/* The multiplier lambda follows quadprog's lambda.ineqlin: the Lagrangian is
 * 1/2 U'GU + F'U + lambda'(Lin U - b), lambda >= 0, one entry per row, zero on rows
 * that are not active.  (The solver works in scaled units, V = U/D with
 * D_j = 1/sqrt(G_jj), rows normalised by rn_i = |Lin_i o D|_2; its multipliers are
 * mu_i = lambda_i rn_i and the export divides by rn_i.)
 * Row order of an MPC step's QP (the oracle's constraints(), the ids of active_ws):
 *   mode 1: rows 0..N-1 are -U_j <= -umin, rows N..2N-1 are U_j <= umax;
 *   modes 2, 3: getWLc's 6N+4 rows: per stage i = 0..N-1 the block [-U_i <= -umin;
 *     U_i <= umax; -x_i <= -xmin (2 rows); x_i <= xmax (2 rows)], then the terminal
 *     [-x_N <= -xmin (2); x_N <= xmax (2)];
 *   mode 3 then adds, for i = 1..N-1, row 6N+4 + 2(i-1) + {0, 1}:
 *     U_i - U_{i-1} <= du_max and U_{i-1} - U_i <= du_max.
 *
 * ntm_qp_device with [x, fval, exitflag, output, lambda] of quadprog: arguments,
 * validation, limits and the results U, exitflag, iters (bit for bit) are
 * ntm_qp_device's.  lambda[m] per scenario (may be NULL when m == 0): for exit flag
 * 1 the multipliers of the certified re-solve (Goldfarb-Idnani's own where the
 * re-solve does not certify and its iterate is returned); every entry 0 for exit
 * flags 0, -2 and -7.  fval (B, may be NULL) = 1/2 U'GU + F'U at the returned U
 * (0 where U = 0). */
int ntm_qp_dual_device(ntm_ctx* ctx, int64_t B, int32_t N, int32_t m,
                       const double* G, const double* F, const double* Lin,
                       const double* b, double* U, int32_t* exitflag,
                       int32_t* iters, double* lambda, double* fval, void* stream);
/* ntm_mpc_step_ws plus, per scenario, lambda[rows(mode)] (the multipliers of the
 * step's last QP; 0 where that QP's exit flag is not 1; may be NULL in mode 0) and
 * rho_qp[3N] (the scheduling rho that QP was built from: the step's rho output is
 * already the post-rollout update).  Every horizon runs on the runtime-N kernels
 * here, N = 10, 20 and 50 included, so the results agree with ntm_mpc_step_ws to
 * the parity tolerances, not bit for bit. */
int ntm_mpc_step_dual(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                      int64_t B, const double* x_k, double* rho, double* U_old,
                      double* U, double* x_pred, double* x_next,
                      int32_t* exitflag, int32_t* inner_iters, int32_t* active_ws,
                      double* lambda, double* rho_qp);
int ntm_mpc_step_dual_device(ntm_ctx* ctx, const ntm_physics* phys,
                             const ntm_config* cfg, int64_t B, const double* x_k,
                             double* rho, double* U_old, double* U, double* x_pred,
                             double* x_next, int32_t* exitflag, int32_t* inner_iters,
                             int32_t* active_ws, double* lambda, double* rho_qp,
                             void* stream);
/* The KKT audit: kkt[4] per scenario from (U, lambda) alone, by arithmetic that
 * shares nothing with the solver but the lift.  With d = D as above, V = U/d,
 * vmax = max(1, max|V|), rn_i as above (1 for a constant row, rn_i = 0),
 * mu_i = lambda_i rn_i, mumax = max(1, max|mu|):
 *   kkt[0] stationarity    max_j |(GU + F + Lin'lambda)_j d_j| / max(1, max_j |F_j d_j|)
 *   kkt[1] primal          max(0, max_i v_i), v_i = (Lin_i U - b_i)/(rn_i vmax) on
 *                          ordinary rows, v_i = -b_i on constant rows
 *   kkt[2] dual            max(0, max_i -mu_i) / mumax
 *   kkt[3] complementarity max_i |mu_i (Lin_i U - b_i)/rn_i| / (mumax vmax), ordinary rows
 * These are the units of the solver's certificate (tolerance 1e-9).  m = 0: only
 * kkt[0] is non-zero.  Non-finite input gives NaN in that scenario's kkt.
 * ntm_qp_kkt_device takes the QP's data (ntm_qp_device's layout; lambda may be NULL
 * when m == 0); ntm_mpc_kkt_device rebuilds the step's QP from x_k[2] and
 * rho_qp[3N] (nominal plasma: a scenario generator's spread is not applied). */
int ntm_qp_kkt_device(ntm_ctx* ctx, int64_t B, int32_t N, int32_t m,
                      const double* G, const double* F, const double* Lin,
                      const double* b, const double* U, const double* lambda,
                      double* kkt, void* stream);
int ntm_mpc_kkt_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                       int64_t B, const double* x_k, const double* rho_qp,
                       const double* U, const double* lambda, double* kkt,
                       void* stream);

/* Synthetic scenarios, counter-based and shard-invariant:
 * x0 for global scenario ids first_id .. first_id+B-1 (host array, 2 per scenario). */
void ntm_scenarios_x0(uint64_t seed, int64_t first_id, int64_t B, double* x0);

/* ---- scenario generator: plasma scenarios and disturbance realisations --- */
/* North_star's "independent plasma scenarios / disturbance realisations"
 * (SURVEY.md §8d): per-scenario plasma parameters j_BS and w_dep (NTM_MPC_Sim.m:5-6,
 * which enter C at :37, B.m:2 and rho3.m:2) and an additive disturbance on the
 * plant step (NTM_MPC_Sim.m:130).  The controller's model is the scenario's own
 * plasma (plant = model, D13); the disturbance is the plant's alone.
 * Counter-based: every value is a function of (seed, global scenario id, time
 * index) only, so any sharding or batching reproduces the same realisations.
 *   u(seed, id, k, ch) = splitmix64^3 chain >> 11, times 2^-53 (uniform [0,1));
 *   n(seed, id, k, c)  = (sum of u at ch = 4c..4c+3 - 2) * sqrt(3): unit variance,
 *                        zero mean, bounded at +-2 sqrt(3) (Irwin-Hall; + and *
 *                        only, so host, device and oracles agree bit for bit);
 *   scenario id: j_BS * (1 + jbs_spread (2 u(id, 0xFFFFFFFF, 0) - 1)),
 *                w_dep * (1 + wdep_spread (2 u(id, 0xFFFFFFFF, 1) - 1));
 *   plant step k: x_{k+1} += [sigma_w n(id, k, 0); sigma_omega n(id, k, 1)]. */
typedef struct {
    uint64_t seed;
    int64_t first_id;    /* global id of the batch's scenario 0 (a shard's offset)   */
    int32_t k0;          /* time index of the next launch's first plant step: the one
                            plant step of ntm_mpc_step*, k0 .. k0+k_sim-1 in ntm_mpc_run* */
    int32_t reserved;    /* must be 0                                                */
    double sigma_w;      /* additive w disturbance per plant step [m], >= 0          */
    double sigma_omega;  /* additive omega disturbance per plant step [rad/s], >= 0  */
    double jbs_spread;   /* relative j_BS spread over scenarios, in [0, 1)           */
    double wdep_spread;  /* relative w_dep spread over scenarios, in [0, 1)          */
} ntm_scenario_gen;
/* Attach a generator to the context (copied): subsequent ntm_mpc_init*,
 * ntm_mpc_step* and ntm_mpc_run* launches use it.  NULL restores the nominal,
 * disturbance-free plant (the reference's own deterministic loop).  The
 * function-level entry points (rho, A/B, lift, cost, getWLc, QP) stay nominal. */
int ntm_ctx_set_scenarios(ntm_ctx* ctx, const ntm_scenario_gen* gen);
/* Host-side samples of the same generator (no GPU): per scenario
 * first_id .. first_id+B-1, out4[4s..4s+3] = (j_BS factor, w_dep factor,
 * n(id, k, 0), n(id, k, 1)). */
void ntm_scenario_sample(const ntm_scenario_gen* gen, int64_t B, int32_t k, double* out4);

/* ---- plant-model mismatch and the offset-free disturbance estimate (ABI v6) ---- */
/* The entry points above give the controller the scenario's own plasma.  Here the
 * model may be the caller's nominal plasma while each plant keeps its own, and the
 * prediction carries an additive disturbance estimate d_hat[2] per scenario (in the
 * state's units, on the model's constant offset C of NTM_MPC_Sim.m:37), corrected each
 * step from the one-step prediction error: offset-free MPC with full state measurement.
 * One step, per scenario:
 *   model  k_m: the caller's ntm_physics when nominal_model is set, else the
 *          scenario's plasma (as ntm_mpc_step*), with C1 + d_hat[0], C2 + d_hat[1].
 *          The lift and the rollout of every LPV iteration use it, so F, the state
 *          rows' right-hand sides and x_pred follow;
 *   plant  k_p: the scenario's plasma when a generator with a spread is attached, else
 *          the caller's; x_next = plant step of k_p at (x_k, U[0]) plus the generator's
 *          disturbance, exactly as ntm_mpc_step*.  The plant never sees d_hat;
 *   e      = x_next - m, m the one-step map of k_m WITHOUT d_hat at (x_k, U[0]) from
 *          rho(x_k), no disturbance (the same expressions as the plant step);
 *   d_hat[i] <- fma(gain, e[i] - d_hat[i], d_hat[i]): one fused multiply-add of the
 *          rounded difference, so every implementation agrees bit for bit (gain 0
 *          freezes d_hat, gain 1 is the deadbeat estimate).  A component whose e is not
 *          finite keeps its value.
 * With nominal_model = 0, gain = 0 and d_hat = 0 the step is ntm_mpc_step_ws's (computed
 * by the runtime-N kernels: every horizon runs on them here, N = 10, 20 and 50 included,
 * as for ntm_mpc_step_dual, so the results agree with the specialised kernels' to the
 * parity tolerances, not bit for bit).  The literal switches D4, D6 and D13
 * (NTM_LITERAL_*) return NTM_E_UNSUPPORTED; NTM_RHO1_SQUARED is allowed.
 * NTM_E_INVALID: NULL obs, reserved != 0, gain outside [0, 1] or NaN, NULL d_hat. */
typedef struct {
    int32_t nominal_model;  /* 1: the controller's model is the caller's ntm_physics; the
                               generator's j_BS / w_dep spreads are the plant's alone.
                               0: model = the scenario's plasma, as ntm_mpc_step*        */
    int32_t reserved;       /* must be 0                                                 */
    double  gain;           /* estimator gain in [0, 1]; 0 freezes d_hat at its input    */
} ntm_observer;
/* ntm_mpc_step_ws with the observer: d_hat[2] per scenario is required, in/out.  When
 * stepping by hand under nominal_model, the initial rho must come from the nominal
 * model too: call ntm_mpc_init* with no generator attached (ntm_ctx_set_scenarios(NULL)),
 * then attach it. */
int ntm_mpc_step_obs(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                     const ntm_observer* obs, int64_t B, const double* x_k, double* rho,
                     double* U_old, double* d_hat, double* U, double* x_pred,
                     double* x_next, int32_t* exitflag, int32_t* inner_iters,
                     int32_t* active_ws);
int ntm_mpc_step_obs_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                            const ntm_observer* obs, int64_t B, const double* x_k,
                            double* rho, double* U_old, double* d_hat, double* U,
                            double* x_pred, double* x_next, int32_t* exitflag,
                            int32_t* inner_iters, int32_t* active_ws, void* stream);
/* ntm_mpc_run with the observer, d_hat kept on chip across the k_sim steps.  d0[2] per
 * scenario is the initial estimate (NULL: zeros).  dk[2(k_sim+1)] per scenario (2 x
 * (k_sim+1), may be NULL): column 0 is d0, column k+1 the estimate after step k.  The
 * initial Rho = repmat(rho(x0)) comes from the model (the nominal one under
 * nominal_model). */
int ntm_mpc_run_obs(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                    const ntm_observer* obs, int64_t B, int32_t k_sim, const double* x0,
                    const double* d0, double* xk, double* uk, double* Uk, double* wpred,
                    double* dk, int32_t* exitflag, int32_t* inner_iters);
int ntm_mpc_run_obs_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                           const ntm_observer* obs, int64_t B, int32_t k_sim,
                           const double* x0, const double* d0, double* xk, double* uk,
                           double* Uk, double* wpred, double* dk, int32_t* exitflag,
                           int32_t* inner_iters, void* stream);

/* ---- measurement noise and a filtered state estimate: output feedback (ABI v7) ---- */
/* The observer entry points above plan from the plant's true state and correct d_hat
 * from the true x_next.  Here the controller sees a noisy measurement only, and three
 * values are carried per scenario: the plant's state x, the estimate x_hat[2] and d_hat[2].
 * One step, per scenario (global id first_id + s, time index k = k0 of the attached
 * generator, k0 + kk inside a run):
 *   controller: the MPC step of ntm_mpc_step_obs (model k_m with C + d_hat in every LPV
 *          iteration) FROM x_hat, not from x: U, x_pred, rho, U_old, the flag and the
 *          iteration count, so the scheduling rho comes from the estimate;
 *   plant  x_next = plant step of k_p at (x, U[0]) plus the generator's disturbance,
 *          exactly as ntm_mpc_step_obs.  It never sees x_hat, d_hat or the measurement noise;
 *   y[i]   = x_next[i] + sigma_y[i] n(seed, id, k, 2 + i): the generator's next two
 *          normal channels (sub-channels 8..15; ntm_meas_sample returns them).  The term
 *          is skipped when sigma_y[i] == 0, as a zero sigma_w is;
 *   m      = k_m's one-step map WITHOUT d_hat and without disturbance at (x_hat, U[0])
 *          from rho(x_hat);
 *   iota[i] = (y[i] - m[i]) - d_hat[i], with the old d_hat;
 *   d_hat[i] <- fma(gain[i], (y[i] - m[i]) - d_hat[i], d_hat[i]), kept where y[i] - m[i]
 *          is not finite (ntm_observer's update);
 *   x_hat[i] <- fma(-kappa[i], iota[i], y[i]), one rounding: (1 - kappa) y + kappa (m +
 *          d_hat).  Where iota[i] is not finite, x_hat[i] <- y[i].
 * With sigma_y = 0, kappa = 0, gain[0] == gain[1] and x_hat == x on input the step is
 * ntm_mpc_step_obs's bit for bit and x_hat comes out equal to x_next.  Every horizon runs
 * on the runtime-N kernels.  The literal switches D4, D6 and D13 return
 * NTM_E_UNSUPPORTED; NTM_RHO1_SQUARED is allowed.  NTM_E_INVALID: NULL est, x_hat or
 * d_hat, reserved != 0, a gain or kappa outside [0, 1] or NaN, a sigma_y negative or not
 * finite, sigma_y != 0 with no generator attached (there is then no seed; a generator
 * with all-zero sigmas and spreads is enough). */
typedef struct {
    int32_t nominal_model;  /* as ntm_observer                                            */
    int32_t reserved;       /* must be 0                                                  */
    double  gain[2];        /* d_hat gain per component (w, omega), in [0, 1]             */
    double  kappa[2];       /* trust in the model per component, in [0, 1]: 0 = x_hat is
                               the measurement                                            */
    double  sigma_y[2];     /* measurement noise std: w [m], omega [rad/s]; finite, >= 0  */
} ntm_estimator;
/* ntm_mpc_step_obs with the estimator.  x_k[2] per scenario is the plant's true state
 * (input); x_hat[2] per scenario is required, in/out, and must not overlap x_k; y[2] per
 * scenario is the measurement of x_next (output, may be NULL). */
int ntm_mpc_step_est(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                     const ntm_estimator* est, int64_t B, const double* x_k, double* rho,
                     double* U_old, double* d_hat, double* x_hat, double* U, double* x_pred,
                     double* x_next, double* y, int32_t* exitflag, int32_t* inner_iters,
                     int32_t* active_ws);
int ntm_mpc_step_est_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                            const ntm_estimator* est, int64_t B, const double* x_k,
                            double* rho, double* U_old, double* d_hat, double* x_hat,
                            double* U, double* x_pred, double* x_next, double* y,
                            int32_t* exitflag, int32_t* inner_iters, int32_t* active_ws,
                            void* stream);
/* ntm_mpc_run_obs with the estimator; x, x_hat and d_hat stay on chip across the k_sim
 * steps.  xhat0[2] per scenario is the initial estimate (NULL: x0).  xhk[2(k_sim+1)] per
 * scenario (may be NULL): column 0 is the initial estimate, column k+1 the estimate after
 * step k.  yk[2 k_sim] per scenario (may be NULL): column k is the measurement of step
 * k's x_next.  The initial Rho = repmat(rho(xhat0)) comes from the model. */
int ntm_mpc_run_est(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                    const ntm_estimator* est, int64_t B, int32_t k_sim, const double* x0,
                    const double* d0, const double* xhat0, double* xk, double* uk,
                    double* Uk, double* wpred, double* dk, double* xhk, double* yk,
                    int32_t* exitflag, int32_t* inner_iters);
int ntm_mpc_run_est_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                           const ntm_estimator* est, int64_t B, int32_t k_sim,
                           const double* x0, const double* d0, const double* xhat0,
                           double* xk, double* uk, double* Uk, double* wpred, double* dk,
                           double* xhk, double* yk, int32_t* exitflag,
                           int32_t* inner_iters, void* stream);
/* ntm_mpc_run_est from a carried state (see ntm_mpc_run_from, whose rules hold here):
 * additionally d_hat[2] and x_hat[2] per scenario, in/out and required; est may differ
 * from call to call too.  For the first call of a loop under nominal_model, ntm_mpc_init
 * runs with no generator attached and from x_hat, as ntm_mpc_step_obs documents.
 * Validation is ntm_mpc_run_est's plus NTM_E_INVALID for a NULL state pointer; x, x_hat
 * and d_hat must not overlap xk, xhk, dk or each other.  The observer loop needs no
 * entry point of its own: with sigma_y = 0, kappa = 0, gain[0] == gain[1] and
 * x_hat == x this is ntm_mpc_run_obs continued, bit for bit. */
int ntm_mpc_run_est_from(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                         const ntm_estimator* est, int64_t B, int32_t k_sim, double* x,
                         double* rho, double* U_old, int32_t* active_ws, double* d_hat,
                         double* x_hat, double* xk, double* uk, double* Uk, double* wpred,
                         double* dk, double* xhk, double* yk, int32_t* exitflag,
                         int32_t* inner_iters);
int ntm_mpc_run_est_from_device(ntm_ctx* ctx, const ntm_physics* phys,
                                const ntm_config* cfg, const ntm_estimator* est, int64_t B,
                                int32_t k_sim, double* x, double* rho, double* U_old,
                                int32_t* active_ws, double* d_hat, double* x_hat, double* xk,
                                double* uk, double* Uk, double* wpred, double* dk,
                                double* xhk, double* yk, int32_t* exitflag,
                                int32_t* inner_iters, void* stream);
/* ---- actuator dead time: delayed inputs and a delay-compensating plan (still ABI v7) ---- */
/* The estimator entry points above apply the input planned at step k at step k.  Here the
 * plant applies the input commanded d = steps sampling periods ago, and one more value is
 * carried per scenario: u_queue[d], the inputs still under way, oldest first (u_queue[0]
 * reaches the plant now, u_queue[d-1] is last step's command).  One step, per scenario:
 *   plan state z = x_hat.  With predict = 1, for j = 0 .. d-1: z <- k_m's one-step map
 *          WITH d_hat (C + d_hat, the model the controller lifts) and without disturbance
 *          at (z, u_queue[j]) from rho(z).  predict = 0 keeps z = x_hat: a controller that
 *          does not know about the delay, for comparison studies;
 *   controller: ntm_mpc_step_est's MPC step FROM z instead of x_hat: U, x_pred, rho, U_old,
 *          the flag, the iteration count and the active sets; u_cmd = U[0];
 *   u_app  = d > 0 ? u_queue[0] : u_cmd;
 *   plant, y, m, d_hat, x_hat: exactly ntm_mpc_step_est's with u_app where it uses U[0]
 *          (x_next = k_p's step at (x, u_app) + disturbance; m = k_m's map without d_hat at
 *          (x_hat, u_app));
 *   queue  u_queue[j] <- u_queue[j+1] for j < d-1, u_queue[d-1] <- u_cmd.
 * With steps = 0 the step is ntm_mpc_step_est's bit for bit, whatever predict is.  The
 * generator's time indices are unchanged, and the initial rho of a loop stays
 * repmat(rho(xhat0)) of the model, so ntm_mpc_init* serves hand-stepped loops as before.
 * A non-finite queue entry makes z non-finite (under predict); that scenario then behaves
 * as one with a non-finite x_hat: flag -7, U = 0, its neighbours untouched.  Every horizon
 * runs on the runtime-N kernels; the queue lives in registers for a whole run.
 * Validation is the estimator entry points' plus NTM_E_INVALID for a NULL delay, steps
 * outside [0, NTM_MAX_DELAY], predict outside {0, 1}, a NULL queue with steps > 0 (uq0 of
 * ntm_mpc_run_dly excepted: NULL = zeros) and a queue that overlaps another argument. */
typedef struct {
    int32_t steps;          /* dead time d in sampling periods, 0 .. NTM_MAX_DELAY          */
    int32_t predict;        /* 1: plan from the state predicted for the command's arrival;
                               0: plan from x_hat                                            */
} ntm_delay;
/* ntm_mpc_step_est with the dead time.  u_queue[steps] per scenario, in/out (may be NULL
 * when steps == 0); x_plan[2] per scenario (output, may be NULL): the z the plan was made
 * from; u_applied[1] per scenario (output, may be NULL): u_app. */
int ntm_mpc_step_dly(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                     const ntm_estimator* est, const ntm_delay* delay, int64_t B,
                     const double* x_k, double* rho, double* U_old, double* d_hat,
                     double* x_hat, double* u_queue, double* U, double* x_pred,
                     double* x_next, double* y, double* x_plan, double* u_applied,
                     int32_t* exitflag, int32_t* inner_iters, int32_t* active_ws);
int ntm_mpc_step_dly_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                            const ntm_estimator* est, const ntm_delay* delay, int64_t B,
                            const double* x_k, double* rho, double* U_old, double* d_hat,
                            double* x_hat, double* u_queue, double* U, double* x_pred,
                            double* x_next, double* y, double* x_plan, double* u_applied,
                            int32_t* exitflag, int32_t* inner_iters, int32_t* active_ws,
                            void* stream);
/* ntm_mpc_run_est with the dead time; the queue stays on chip across the k_sim steps.
 * uq0[steps] per scenario is the initial queue (NULL: zeros, power off until the first
 * command arrives).  uak[k_sim] per scenario (may be NULL): the applied input of step k;
 * uk stays the commanded U[0], so uak[k + steps] == uk[k].  xpk[2 k_sim] per scenario (may
 * be NULL): the plan state z of step k. */
int ntm_mpc_run_dly(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                    const ntm_estimator* est, const ntm_delay* delay, int64_t B,
                    int32_t k_sim, const double* x0, const double* d0, const double* xhat0,
                    const double* uq0, double* xk, double* uk, double* Uk, double* wpred,
                    double* dk, double* xhk, double* yk, double* uak, double* xpk,
                    int32_t* exitflag, int32_t* inner_iters);
int ntm_mpc_run_dly_device(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                           const ntm_estimator* est, const ntm_delay* delay, int64_t B,
                           int32_t k_sim, const double* x0, const double* d0,
                           const double* xhat0, const double* uq0, double* xk, double* uk,
                           double* Uk, double* wpred, double* dk, double* xhk, double* yk,
                           double* uak, double* xpk, int32_t* exitflag,
                           int32_t* inner_iters, void* stream);
/* ntm_mpc_run_est_from with the dead time (ntm_mpc_run_from's rules hold): u_queue[steps]
 * per scenario is carried in and out with the rest of the state, required when steps > 0.
 * The same bits come out whether k steps run in one call or split over several.  steps
 * must not change between the chunks of one loop (the queue's length is the delay);
 * predict and est may. */
int ntm_mpc_run_dly_from(ntm_ctx* ctx, const ntm_physics* phys, const ntm_config* cfg,
                         const ntm_estimator* est, const ntm_delay* delay, int64_t B,
                         int32_t k_sim, double* x, double* rho, double* U_old,
                         int32_t* active_ws, double* d_hat, double* x_hat, double* u_queue,
                         double* xk, double* uk, double* Uk, double* wpred, double* dk,
                         double* xhk, double* yk, double* uak, double* xpk,
                         int32_t* exitflag, int32_t* inner_iters);
int ntm_mpc_run_dly_from_device(ntm_ctx* ctx, const ntm_physics* phys,
                                const ntm_config* cfg, const ntm_estimator* est,
                                const ntm_delay* delay, int64_t B, int32_t k_sim, double* x,
                                double* rho, double* U_old, int32_t* active_ws,
                                double* d_hat, double* x_hat, double* u_queue, double* xk,
                                double* uk, double* Uk, double* wpred, double* dk,
                                double* xhk, double* yk, double* uak, double* xpk,
                                int32_t* exitflag, int32_t* inner_iters, void* stream);
/* Host-side unit samples of the measurement noise for scenarios first_id .. first_id + B
 * - 1 at time index k (out2: 2 per scenario: n(id, k, 2), n(id, k, 3)); the sibling of
 * ntm_scenario_sample, the same code the kernels run. */
void ntm_meas_sample(const ntm_scenario_gen* gen, int64_t B, int32_t k, double* out2);

#ifdef __cplusplus
}
#endif
#endif /* NTM_MPC_H */
