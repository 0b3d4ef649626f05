/*
 * ntm_mpc_mex.c — MATLAB MEX gateway over the C-ABI in include/ntm_mpc.h.
 *
 * Replaces, for a batch of B scenarios, the body of the receding-horizon loop
 * of NTM_MPC_Sim.m (lines 94-130: the LPV iteration, quadprog call and plant
 * step) or the whole closed loop (lines 80-131).  Build, where MATLAB exists:
 *
 *   mex -R2018a -I../../include ntm_mpc_mex.c \
 *       -L../../mpc-ntm-control_amd/lib -lntm_mpc
 *
 * Calls (every batched array is E-by-B: one column per scenario, which is the
 * ABI's scenario-major layout [s*E + e] in MATLAB's column-major storage, so
 * arrays pass through without copies):
 *
 *   [U, x_pred, x_next, exitflag, iters, rho, Uold, ws, lambda, rho_qp] = ...
 *       ntm_mpc_mex('step', x_k, rho, Uold, cfg[, ws])
 *         x_k  2-by-B        current state [w; omega]           (xk(:,k))
 *         rho  3N-by-B       Rho(:) per scenario                (:63-65,116)
 *         Uold N-by-B        +Inf on the first step (D14)
 *         ws   2(N+1)-by-B   optional int32 warm-start workspace (start with
 *                            -1 everywhere; pass the returned one back next step)
 *       outputs: U N-by-B, x_pred 2(N+1)-by-B, x_next 2-by-B, exitflag and
 *       iters 1-by-B.  Asked for more than eight outputs, the step also returns
 *       lambda rows(mode)-by-B, the last QP's multipliers (quadprog's
 *       lambda.ineqlin, the row order of include/ntm_mpc.h), and rho_qp 3N-by-B,
 *       the scheduling rho that QP was built from (ntm_mpc_step_dual: the
 *       runtime-horizon kernels, results to the parity tolerances); with eight
 *       or fewer it is ntm_mpc_step_ws as before
 *   [rho, Uold] = ntm_mpc_mex('init', x0, cfg)                 (:63-65, :86)
 *   [xk, uk, Uk, wpred, exitflag, iters] = ntm_mpc_mex('run', x0, k_sim, cfg)
 *       outputs 2(k_sim+1)-by-B, k_sim-by-B, N k_sim-by-B, (N+1) k_sim-by-B,
 *       k_sim-by-B, k_sim-by-B (per scenario column: xk(:), uk, Uk(:), ...)
 *   [U, x_pred, x_next, exitflag, iters, rho, Uold, ws, d_hat] = ...
 *       ntm_mpc_mex('step_obs', x_k, rho, Uold, d_hat, obs[, cfg[, ws]])
 *       'step' with plant-model mismatch and the disturbance estimate
 *       (ntm_mpc_step_obs, ABI v6): obs is a struct with nominal_model (1: the
 *       controller's model is the nominal plasma, the 'scenarios' spreads are the
 *       plants' alone) and gain in [0, 1]; d_hat 2-by-B is the carried estimate
 *       (zeros to start), returned updated as output 9.  Under nominal_model call
 *       'init' before 'scenarios', so that the initial rho is the nominal model's.
 *   [xk, uk, Uk, wpred, exitflag, iters, dk] = ...
 *       ntm_mpc_mex('run_obs', x0, k_sim, obs[, cfg[, d0]])
 *       'run' with the observer (ntm_mpc_run_obs): d0 2-by-B the initial estimate
 *       (omitted: zeros); dk 2(k_sim+1)-by-B, column 1 of each scenario's
 *       2-by-(k_sim+1) history is d0, column k+1 the estimate after step k.
 *   [U, x_pred, x_next, exitflag, iters, rho, Uold, ws, d_hat, x_hat, y] = ...
 *       ntm_mpc_mex('step_est', x_k, rho, Uold, d_hat, x_hat, est[, cfg[, ws]])
 *       'step_obs' with output feedback (ntm_mpc_step_est, ABI v7): the controller
 *       plans from the estimate x_hat 2-by-B while the plant steps from its true
 *       state x_k; est is a struct with any of nominal_model, gain, kappa, sigma_y
 *       (ntm_estimator; the last three [w omega] pairs, a scalar sets both, missing
 *       fields are 0).  d_hat and x_hat come back updated as outputs 9 and 10, y
 *       2-by-B is the noisy measurement of x_next.  sigma_y ~= 0 needs 'scenarios'
 *       (any gen struct, all zeros included) for the seed.
 *   [xk, uk, Uk, wpred, exitflag, iters, dk, xhk, yk] = ...
 *       ntm_mpc_mex('run_est', x0, k_sim, est[, cfg[, d0[, xhat0]]])
 *       'run_obs' with the estimator (ntm_mpc_run_est): d0 and xhat0 2-by-B
 *       (omitted or []: zeros, x0); xhk 2(k_sim+1)-by-B, the estimate's history
 *       from xhat0 on; yk 2 k_sim-by-B, the measurements.
 *   [xk, uk, Uk, wpred, exitflag, iters, x, rho, Uold, ws] = ...
 *       ntm_mpc_mex('run_from', x, rho, Uold, ws, k_sim[, cfg])
 *       'run' from a carried state (ntm_mpc_run_from, NTM_MPC_HAS_RUN_FROM): x 2-by-B,
 *       rho, Uold and the int32 ws as for 'step' (a loop's first call: 'init' and -1
 *       everywhere); they come back as outputs 7 to 10 holding the state after the
 *       last step, to be passed to the next call, so a loop can run in chunks with
 *       cfg or 'scenarios' changed in between (advance gen.k0 by the steps done).
 *       k_sim >= 0; the histories are those of 'run', xk's first column the input x.
 *   [xk, uk, Uk, wpred, exitflag, iters, dk, xhk, yk, x, rho, Uold, ws, d_hat, x_hat] = ...
 *       ntm_mpc_mex('run_est_from', x, rho, Uold, ws, d_hat, x_hat, k_sim, est[, cfg])
 *       'run_est' from a carried state (ntm_mpc_run_est_from): d_hat and x_hat 2-by-B
 *       are carried too; the state comes back as outputs 10 to 15.
 *   [U, x_pred, x_next, exitflag, iters, rho, Uold, ws, d_hat, x_hat, y, u_queue, x_plan, u_app] = ...
 *       ntm_mpc_mex('step_dly', x_k, rho, Uold, d_hat, x_hat, u_queue, est, dly[, cfg[, ws]])
 *       'step_est' with an actuator dead time (ntm_mpc_step_dly, NTM_MPC_HAS_INPUT_DELAY):
 *       dly is a struct with steps (0 .. 8) and predict (missing: 1); u_queue steps-by-B
 *       holds the inputs under way, oldest first ([] when steps is 0), and comes back
 *       shifted with the new command at its end as output 12; x_plan 2-by-B is the state
 *       the plan was made from, u_app 1-by-B the input the plant received.
 *   [xk, uk, Uk, wpred, exitflag, iters, dk, xhk, yk, uak, xpk] = ...
 *       ntm_mpc_mex('run_dly', x0, k_sim, est, dly[, cfg[, d0[, xhat0[, uq0]]]])
 *       'run_est' with the dead time (ntm_mpc_run_dly): uq0 steps-by-B the initial queue
 *       (omitted or []: zeros); uak k_sim-by-B the applied inputs (uk stays the commanded
 *       ones), xpk 2 k_sim-by-B the plan states.
 *   [xk, uk, Uk, wpred, exitflag, iters, dk, xhk, yk, uak, xpk, x, rho, Uold, ws, d_hat, x_hat, u_queue] = ...
 *       ntm_mpc_mex('run_dly_from', x, rho, Uold, ws, d_hat, x_hat, u_queue, k_sim, est, dly[, cfg])
 *       'run_dly' from a carried state (ntm_mpc_run_dly_from): the queue is carried too;
 *       the state comes back as outputs 12 to 18.  dly.steps must not change between the
 *       chunks of one loop.
 *   ntm_mpc_mex('scenarios', gen)                               
 *       gen struct with any of seed, first_id, k0, sigma_w, sigma_omega,
 *       jbs_spread, wdep_spread (ntm_scenario_gen): per-scenario plasma and
 *       plant disturbances for the following init/step/run calls; [] = off.
 *       With 'step', set k0 to the step's time index before each call.
 *   ntm_mpc_mex('close')
 *
 * cfg is an optional struct with any of the fields N, i_sim, mode, flags, Ts,
 * xmin, xmax, umin, umax, Q (2x2), r, epsilon, du_max, Ru (input weight, ABI v5);
 * missing fields take the
 * reference literals (ntm_config_default).  Library errors become MATLAB
 * errors (ntm:...); solver outcomes are returned in exitflag (quadprog codes,
 * NTM_MPC_Sim.m:98-103), never raised.
 */
#include <string.h>

#include "mex.h"
#include "ntm_mpc.h"

static ntm_ctx* g_ctx = NULL;

static void release(void) {
    if (g_ctx) {
        ntm_ctx_destroy(g_ctx);
        g_ctx = NULL;
    }
}

static void check(int rc, const char* what) {
    if (rc != NTM_OK) {
        mexErrMsgIdAndTxt("ntm:library", "%s failed (%d): %s", what, rc, g_ctx ? ntm_last_error(g_ctx) : "no context");
    }
}

static ntm_ctx* ctx(void) {
    if (!g_ctx) {
        check(ntm_ctx_create(&g_ctx, 0), "ntm_ctx_create");
        mexAtExit(release);
    }
    return g_ctx;
}

static double scalar_field(const mxArray* s, const char* name, double dflt) {
    const mxArray* f = s ? mxGetField(s, 0, name) : NULL;
    return (f && mxIsDouble(f) && mxGetNumberOfElements(f) >= 1) ? mxGetDoubles(f)[0] : dflt;
}

static void vec_field(const mxArray* s, const char* name, double* dst, size_t n) {
    const mxArray* f = s ? mxGetField(s, 0, name) : NULL;
    if (!f) return;
    if (!mxIsDouble(f) || mxGetNumberOfElements(f) != n) mexErrMsgIdAndTxt("ntm:cfg", "cfg.%s must have %d doubles", name, (int)n);
    memcpy(dst, mxGetDoubles(f), n * sizeof(double));
}

static ntm_config read_cfg(const mxArray* s) {
    ntm_config c;
    if (s && !mxIsStruct(s)) mexErrMsgIdAndTxt("ntm:cfg", "cfg must be a struct");
    ntm_config_default(&c, (int32_t)scalar_field(s, "N", 20));
    c.i_sim = (int32_t)scalar_field(s, "i_sim", c.i_sim);
    c.mode = (int32_t)scalar_field(s, "mode", c.mode);
    c.flags = (int32_t)scalar_field(s, "flags", c.flags);
    c.Ts = scalar_field(s, "Ts", c.Ts);
    c.umin = scalar_field(s, "umin", c.umin);
    c.umax = scalar_field(s, "umax", c.umax);
    c.epsilon = scalar_field(s, "epsilon", c.epsilon);
    c.du_max = scalar_field(s, "du_max", c.du_max);
    c.Ru = scalar_field(s, "Ru", c.Ru);
    vec_field(s, "xmin", c.xmin, 2);
    vec_field(s, "xmax", c.xmax, 2);
    vec_field(s, "r", c.r, 2);
    if (s && mxGetField(s, 0, "Q")) {   /* MATLAB 2x2 is column-major; the ABI's Q is row-major */
        double q[4];
        vec_field(s, "Q", q, 4);
        c.Q[0] = q[0]; c.Q[1] = q[2]; c.Q[2] = q[1]; c.Q[3] = q[3];
    }
    return c;
}

static const double* in_matrix(const mxArray* a, size_t rows, size_t cols, const char* name) {
    if (!mxIsDouble(a) || mxIsComplex(a) || mxGetM(a) != rows || mxGetN(a) != cols)
        mexErrMsgIdAndTxt("ntm:arg", "%s must be a real %d-by-%d double array", name, (int)rows, (int)cols);
    return mxGetDoubles(a);
}

#define D(a) mxGetDoubles(a)
#define I(a) mxGetInt32s(a)

/* an optional 2-by-B input: omitted or [] gives NULL */
static const double* opt_matrix(int nrhs, const mxArray* prhs[], int i, size_t B, const char* name) {
    if (nrhs <= i || (mxIsDouble(prhs[i]) && mxGetNumberOfElements(prhs[i]) == 0)) return NULL;
    return in_matrix(prhs[i], 2, B, name);
}

/* the int32 2(N+1)-by-B warm-start workspace (the '*_from' commands require one) */
static void in_ws(const mxArray* w, size_t N, size_t B) {
    if (!mxIsInt32(w) || mxGetM(w) != 2 * (N + 1) || mxGetN(w) != B)
        mexErrMsgIdAndTxt("ntm:arg", "ws must be an int32 %d-by-%d array", (int)(2 * (N + 1)), (int)B);
}

/* the workspace as an output (value semantics): a copy of the caller's, or, where the
 * command was given none (w == NULL), an empty one, -1 everywhere */
static mxArray* dup_ws(const mxArray* w, size_t N, size_t B) {
    if (w) {
        in_ws(w, N, B);
        return mxDuplicateArray(w);
    }
    mxArray* ws = mxCreateNumericMatrix(2 * (N + 1), B, mxINT32_CLASS, mxREAL);
    for (size_t i = 0; i < B * 2 * (N + 1); ++i) I(ws)[i] = -1;
    return ws;
}

/* k_sim of the 'run*' commands (>= 1) and of the '*_from' commands (a scalar >= 0) */
static int in_ksim_run(const mxArray* a) {
    const int k = (int)mxGetScalar(a);
    if (k < 1) mexErrMsgIdAndTxt("ntm:arg", "k_sim must be >= 1");
    return k;
}

static int in_ksim(const mxArray* a) {
    if (!mxIsDouble(a) || mxGetNumberOfElements(a) != 1 || !(mxGetScalar(a) >= 0))
        mexErrMsgIdAndTxt("ntm:arg", "k_sim must be a scalar >= 0");
    return (int)mxGetScalar(a);
}

/* The 'step*' commands' own outputs: U N-by-B, x_pred 2(N+1)-by-B, x_next 2-by-B, exitflag
 * and iters 1-by-B are outputs 1 to 5 of each; y 2-by-B ('step_est', 'step_dly'), x_plan
 * 2-by-B and u_app 1-by-B ('step_dly') follow the returned state, where each command says. */
typedef struct {
    mxArray *U, *xp, *xn, *fl, *it, *y, *z, *ua;
} step_out;

static step_out new_step_out(size_t N, size_t B, int est, int dly) {
    step_out o = {mxCreateDoubleMatrix(N, B, mxREAL), mxCreateDoubleMatrix(2 * (N + 1), B, mxREAL),
                  mxCreateDoubleMatrix(2, B, mxREAL), mxCreateNumericMatrix(1, B, mxINT32_CLASS, mxREAL),
                  mxCreateNumericMatrix(1, B, mxINT32_CLASS, mxREAL), NULL, NULL, NULL};
    if (est) o.y = mxCreateDoubleMatrix(2, B, mxREAL);
    if (dly) {
        o.z = mxCreateDoubleMatrix(2, B, mxREAL);
        o.ua = mxCreateDoubleMatrix(1, B, mxREAL);
    }
    return o;
}

/* The closed-loop histories of the 'run*' commands for k steps.  The fields stand in the
 * MEX output order, which every 'run*' command shares: xk, uk, Uk, wpred, exitflag, iters
 * (outputs 1 to 6), then dk (observer), xhk and yk (estimator), uak and xpk (dead time); a
 * '*_from' command appends its carried state.  It is not the C-ABI's order: there exitflag
 * and iters come last, after the extras. */
typedef struct {
    mxArray *xk, *uk, *Uk, *wp, *fl, *it, *dk, *xhk, *yk, *uak, *xpk;
} loop_out;

static loop_out new_loop_out(int k_sim, size_t N, size_t B, int obs, int est, int dly) {
    const size_t k = (size_t)k_sim;
    loop_out o = {mxCreateDoubleMatrix(2 * (k + 1), B, mxREAL), mxCreateDoubleMatrix(k, B, mxREAL),
                  mxCreateDoubleMatrix(N * k, B, mxREAL), mxCreateDoubleMatrix((N + 1) * k, B, mxREAL),
                  mxCreateNumericMatrix(k, B, mxINT32_CLASS, mxREAL),
                  mxCreateNumericMatrix(k, B, mxINT32_CLASS, mxREAL), NULL, NULL, NULL, NULL, NULL};
    if (obs) o.dk = mxCreateDoubleMatrix(2 * (k + 1), B, mxREAL);
    if (est) {
        o.xhk = mxCreateDoubleMatrix(2 * (k + 1), B, mxREAL);
        o.yk = mxCreateDoubleMatrix(2 * k, B, mxREAL);
    }
    if (dly) {
        o.uak = mxCreateDoubleMatrix(k, B, mxREAL);
        o.xpk = mxCreateDoubleMatrix(2 * k, B, mxREAL);
    }
    return o;
}

/* hand a command's n outputs to plhs: as many as the caller asked for (one at least), the
 * rest destroyed */
static void put_outs(int nlhs, mxArray* plhs[], mxArray** outs, int n) {
    for (int i = 0; i < n; ++i) {
        if (i < (nlhs > 0 ? nlhs : 1)) plhs[i] = outs[i];
        else mxDestroyArray(outs[i]);
    }
}

static void do_step(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 4) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('step', x_k, rho, Uold[, cfg[, ws]])");
    const ntm_config c = read_cfg(nrhs > 4 ? prhs[4] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x = in_matrix(prhs[1], 2, B, "x_k");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    /* value semantics: rho / Uold are updated in copies returned as outputs 6-7 */
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    const step_out o = new_step_out(N, B, 0, 0);
    mxArray* ws = dup_ws(nrhs > 5 ? prhs[5] : NULL, N, B);
    mxArray* lam = NULL;
    mxArray* rq = NULL;
    if (nlhs > 8) {
        const size_t m = c.mode == NTM_MODE_NONE ? 0
                         : c.mode == NTM_MODE_BOX ? 2 * N
                         : c.mode == NTM_MODE_FULL_DU ? 8 * N + 2 : 6 * N + 4;
        lam = mxCreateDoubleMatrix(m, B, mxREAL);
        rq = mxCreateDoubleMatrix(3 * N, B, mxREAL);
        check(ntm_mpc_step_dual(ctx(), &p, &c, (int64_t)B, x, D(rho), D(uold), D(o.U), D(o.xp), D(o.xn), I(o.fl),
                                I(o.it), I(ws), m ? D(lam) : NULL, D(rq)),
              "ntm_mpc_step_dual");
    } else {
        check(ntm_mpc_step_ws(ctx(), &p, &c, (int64_t)B, x, D(rho), D(uold), D(o.U), D(o.xp), D(o.xn), I(o.fl),
                              I(o.it), I(ws)),
              "ntm_mpc_step_ws");
    }
    mxArray* outs[10] = {o.U, o.xp, o.xn, o.fl, o.it, rho, uold, ws, lam, rq};
    put_outs(nlhs, plhs, outs, lam ? 10 : 8);
}

static void do_init(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 2) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('init', x0[, cfg])");
    const ntm_config c = read_cfg(nrhs > 2 ? prhs[2] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x0 = in_matrix(prhs[1], 2, B, "x0");
    mxArray* rho = mxCreateDoubleMatrix(3 * N, B, mxREAL);
    mxArray* uold = mxCreateDoubleMatrix(N, B, mxREAL);
    check(ntm_mpc_init(ctx(), &p, &c, (int64_t)B, x0, D(rho), D(uold)), "ntm_mpc_init");
    plhs[0] = rho;
    if (nlhs > 1) plhs[1] = uold;
    else mxDestroyArray(uold);
}

static void do_run(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 3) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('run', x0, k_sim[, cfg])");
    const ntm_config c = read_cfg(nrhs > 3 ? prhs[3] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x0 = in_matrix(prhs[1], 2, B, "x0");
    const int k = in_ksim_run(prhs[2]);
    const loop_out o = new_loop_out(k, N, B, 0, 0, 0);
    check(ntm_mpc_run(ctx(), &p, &c, (int64_t)B, k, x0, D(o.xk), D(o.uk), D(o.Uk), D(o.wp), I(o.fl), I(o.it)),
          "ntm_mpc_run");
    mxArray* outs[6] = {o.xk, o.uk, o.Uk, o.wp, o.fl, o.it};
    put_outs(nlhs, plhs, outs, 6);
}

/* obs struct with any of nominal_model, gain (ntm_observer); missing fields are 0 */
static ntm_observer read_obs(const mxArray* s) {
    ntm_observer o;
    if (!s || !mxIsStruct(s)) mexErrMsgIdAndTxt("ntm:arg", "obs must be a struct with nominal_model and gain");
    memset(&o, 0, sizeof o);
    o.nominal_model = scalar_field(s, "nominal_model", 0.0) != 0.0;
    o.gain = scalar_field(s, "gain", 0.0);
    return o;
}

/* 'step' with the observer (ntm_mpc_step_obs): d_hat goes in after Uold and comes
 * back, updated, as output 9 */
static void do_step_obs(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 6) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('step_obs', x_k, rho, Uold, d_hat, obs[, cfg[, ws]])");
    const ntm_observer ob = read_obs(prhs[5]);
    const ntm_config c = read_cfg(nrhs > 6 ? prhs[6] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x = in_matrix(prhs[1], 2, B, "x_k");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    in_matrix(prhs[4], 2, B, "d_hat");
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    mxArray* dh = mxDuplicateArray(prhs[4]);
    const step_out o = new_step_out(N, B, 0, 0);
    mxArray* ws = dup_ws(nrhs > 7 ? prhs[7] : NULL, N, B);
    check(ntm_mpc_step_obs(ctx(), &p, &c, &ob, (int64_t)B, x, D(rho), D(uold), D(dh), D(o.U), D(o.xp), D(o.xn), I(o.fl),
                           I(o.it), I(ws)),
          "ntm_mpc_step_obs");
    mxArray* outs[9] = {o.U, o.xp, o.xn, o.fl, o.it, rho, uold, ws, dh};
    put_outs(nlhs, plhs, outs, 9);
}

/* 'run' with the observer (ntm_mpc_run_obs): dk is output 7 */
static void do_run_obs(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 4) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('run_obs', x0, k_sim, obs[, cfg[, d0]])");
    const ntm_observer ob = read_obs(prhs[3]);
    const ntm_config c = read_cfg(nrhs > 4 ? prhs[4] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x0 = in_matrix(prhs[1], 2, B, "x0");
    const double* d0 = nrhs > 5 ? in_matrix(prhs[5], 2, B, "d0") : NULL;
    const int k = in_ksim_run(prhs[2]);
    const loop_out o = new_loop_out(k, N, B, 1, 0, 0);
    check(ntm_mpc_run_obs(ctx(), &p, &c, &ob, (int64_t)B, k, x0, d0, D(o.xk), D(o.uk), D(o.Uk), D(o.wp), D(o.dk),
                          I(o.fl), I(o.it)),
          "ntm_mpc_run_obs");
    mxArray* outs[7] = {o.xk, o.uk, o.Uk, o.wp, o.fl, o.it, o.dk};
    put_outs(nlhs, plhs, outs, 7);
}

/* est struct with any of nominal_model, gain, kappa, sigma_y (ntm_estimator); the last
 * three are [w omega] pairs, a scalar sets both components; missing fields are 0 */
static void pair_field(const mxArray* s, const char* name, double* dst) {
    const mxArray* f = mxGetField(s, 0, name);
    dst[0] = dst[1] = 0.0;
    if (!f) return;
    const size_t n = mxIsDouble(f) ? mxGetNumberOfElements(f) : 0;
    if (n != 1 && n != 2) mexErrMsgIdAndTxt("ntm:arg", "est.%s must have 1 or 2 doubles", name);
    dst[0] = mxGetDoubles(f)[0];
    dst[1] = mxGetDoubles(f)[n - 1];
}

static ntm_estimator read_est(const mxArray* s) {
    ntm_estimator e;
    if (!s || !mxIsStruct(s))
        mexErrMsgIdAndTxt("ntm:arg", "est must be a struct with nominal_model, gain, kappa and sigma_y");
    memset(&e, 0, sizeof e);
    e.nominal_model = scalar_field(s, "nominal_model", 0.0) != 0.0;
    pair_field(s, "gain", e.gain);
    pair_field(s, "kappa", e.kappa);
    pair_field(s, "sigma_y", e.sigma_y);
    return e;
}

/* 'step_obs' with the estimator (ntm_mpc_step_est): x_hat goes in after d_hat; d_hat,
 * x_hat and the measurement y are outputs 9 to 11 */
static void do_step_est(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 7)
        mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('step_est', x_k, rho, Uold, d_hat, x_hat, est[, cfg[, ws]])");
    const ntm_estimator e = read_est(prhs[6]);
    const ntm_config c = read_cfg(nrhs > 7 ? prhs[7] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x = in_matrix(prhs[1], 2, B, "x_k");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    in_matrix(prhs[4], 2, B, "d_hat");
    in_matrix(prhs[5], 2, B, "x_hat");
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    mxArray* dh = mxDuplicateArray(prhs[4]);
    mxArray* xh = mxDuplicateArray(prhs[5]);
    const step_out o = new_step_out(N, B, 1, 0);
    mxArray* ws = dup_ws(nrhs > 8 ? prhs[8] : NULL, N, B);
    check(ntm_mpc_step_est(ctx(), &p, &c, &e, (int64_t)B, x, D(rho), D(uold), D(dh), D(xh), D(o.U), D(o.xp), D(o.xn),
                           D(o.y), I(o.fl), I(o.it), I(ws)),
          "ntm_mpc_step_est");
    mxArray* outs[11] = {o.U, o.xp, o.xn, o.fl, o.it, rho, uold, ws, dh, xh, o.y};
    put_outs(nlhs, plhs, outs, 11);
}

/* 'run_obs' with the estimator (ntm_mpc_run_est): dk, xhk and yk are outputs 7 to 9 */
static void do_run_est(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 4) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('run_est', x0, k_sim, est[, cfg[, d0[, xhat0]]])");
    const ntm_estimator e = read_est(prhs[3]);
    const ntm_config c = read_cfg(nrhs > 4 ? prhs[4] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x0 = in_matrix(prhs[1], 2, B, "x0");
    const double* d0 = opt_matrix(nrhs, prhs, 5, B, "d0");
    const double* h0 = opt_matrix(nrhs, prhs, 6, B, "xhat0");
    const int k = in_ksim_run(prhs[2]);
    const loop_out o = new_loop_out(k, N, B, 1, 1, 0);
    check(ntm_mpc_run_est(ctx(), &p, &c, &e, (int64_t)B, k, x0, d0, h0, D(o.xk), D(o.uk), D(o.Uk), D(o.wp), D(o.dk),
                          D(o.xhk), D(o.yk), I(o.fl), I(o.it)),
          "ntm_mpc_run_est");
    mxArray* outs[9] = {o.xk, o.uk, o.Uk, o.wp, o.fl, o.it, o.dk, o.xhk, o.yk};
    put_outs(nlhs, plhs, outs, 9);
}

/* 'run' from a carried state (ntm_mpc_run_from): the state is outputs 7 to 10 */
static void do_run_from(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 6) mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('run_from', x, rho, Uold, ws, k_sim[, cfg])");
    const ntm_config c = read_cfg(nrhs > 6 ? prhs[6] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    in_matrix(prhs[1], 2, B, "x");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    in_ws(prhs[4], N, B);
    const int k = in_ksim(prhs[5]);
    mxArray* x = mxDuplicateArray(prhs[1]);
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    mxArray* ws = mxDuplicateArray(prhs[4]);
    const loop_out o = new_loop_out(k, N, B, 0, 0, 0);
    check(ntm_mpc_run_from(ctx(), &p, &c, (int64_t)B, k, D(x), D(rho), D(uold), I(ws), D(o.xk), D(o.uk), D(o.Uk),
                           D(o.wp), I(o.fl), I(o.it)),
          "ntm_mpc_run_from");
    mxArray* outs[10] = {o.xk, o.uk, o.Uk, o.wp, o.fl, o.it, x, rho, uold, ws};
    put_outs(nlhs, plhs, outs, 10);
}

/* 'run_est' from a carried state (ntm_mpc_run_est_from): the state is outputs 10 to 15 */
static void do_run_est_from(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 9)
        mexErrMsgIdAndTxt("ntm:arg",
                          "usage: ntm_mpc_mex('run_est_from', x, rho, Uold, ws, d_hat, x_hat, k_sim, est[, cfg])");
    const ntm_estimator e = read_est(prhs[8]);
    const ntm_config c = read_cfg(nrhs > 9 ? prhs[9] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    in_matrix(prhs[1], 2, B, "x");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    in_ws(prhs[4], N, B);
    in_matrix(prhs[5], 2, B, "d_hat");
    in_matrix(prhs[6], 2, B, "x_hat");
    const int k = in_ksim(prhs[7]);
    mxArray* x = mxDuplicateArray(prhs[1]);
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    mxArray* ws = mxDuplicateArray(prhs[4]);
    mxArray* dh = mxDuplicateArray(prhs[5]);
    mxArray* xh = mxDuplicateArray(prhs[6]);
    const loop_out o = new_loop_out(k, N, B, 1, 1, 0);
    check(ntm_mpc_run_est_from(ctx(), &p, &c, &e, (int64_t)B, k, D(x), D(rho), D(uold), I(ws), D(dh), D(xh), D(o.xk),
                               D(o.uk), D(o.Uk), D(o.wp), D(o.dk), D(o.xhk), D(o.yk), I(o.fl), I(o.it)),
          "ntm_mpc_run_est_from");
    mxArray* outs[15] = {o.xk, o.uk, o.Uk, o.wp, o.fl, o.it, o.dk, o.xhk, o.yk, x, rho, uold, ws, dh, xh};
    put_outs(nlhs, plhs, outs, 15);
}

/* dly struct with steps (0 .. NTM_MAX_DELAY) and predict (missing: 1) (ntm_delay) */
static ntm_delay read_dly(const mxArray* s) {
    ntm_delay d;
    if (!s || !mxIsStruct(s)) mexErrMsgIdAndTxt("ntm:arg", "dly must be a struct with steps and predict");
    d.steps = (int32_t)scalar_field(s, "steps", 0.0);
    d.predict = (int32_t)scalar_field(s, "predict", 1.0);
    if (d.steps < 0 || d.steps > NTM_MAX_DELAY)
        mexErrMsgIdAndTxt("ntm:arg", "dly.steps must be in 0 .. %d", (int)NTM_MAX_DELAY);
    return d;
}

/* the queue of pending inputs, steps-by-B; with steps == 0 any empty array will do */
static void in_queue(const mxArray* a, size_t steps, size_t B, const char* name) {
    if (steps == 0 && mxIsDouble(a) && mxGetNumberOfElements(a) == 0) return;
    in_matrix(a, steps, B, name);
}

/* 'step_est' with the dead time (ntm_mpc_step_dly): u_queue goes in after x_hat, dly after
 * est; the shifted queue, the plan state and the applied input are outputs 12 to 14 */
static void do_step_dly(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 9)
        mexErrMsgIdAndTxt("ntm:arg",
                          "usage: ntm_mpc_mex('step_dly', x_k, rho, Uold, d_hat, x_hat, u_queue, est, dly[, cfg[, ws]])");
    const ntm_estimator e = read_est(prhs[7]);
    const ntm_delay d = read_dly(prhs[8]);
    const ntm_config c = read_cfg(nrhs > 9 ? prhs[9] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x = in_matrix(prhs[1], 2, B, "x_k");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    in_matrix(prhs[4], 2, B, "d_hat");
    in_matrix(prhs[5], 2, B, "x_hat");
    in_queue(prhs[6], (size_t)d.steps, B, "u_queue");
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    mxArray* dh = mxDuplicateArray(prhs[4]);
    mxArray* xh = mxDuplicateArray(prhs[5]);
    mxArray* uq = d.steps ? mxDuplicateArray(prhs[6]) : mxCreateDoubleMatrix(0, B, mxREAL);
    const step_out o = new_step_out(N, B, 1, 1);
    mxArray* ws = dup_ws(nrhs > 10 ? prhs[10] : NULL, N, B);
    check(ntm_mpc_step_dly(ctx(), &p, &c, &e, &d, (int64_t)B, x, D(rho), D(uold), D(dh), D(xh), d.steps ? D(uq) : NULL,
                           D(o.U), D(o.xp), D(o.xn), D(o.y), D(o.z), D(o.ua), I(o.fl), I(o.it), I(ws)),
          "ntm_mpc_step_dly");
    mxArray* outs[14] = {o.U, o.xp, o.xn, o.fl, o.it, rho, uold, ws, dh, xh, o.y, uq, o.z, o.ua};
    put_outs(nlhs, plhs, outs, 14);
}

/* 'run_est' with the dead time (ntm_mpc_run_dly): uak and xpk are outputs 10 and 11 */
static void do_run_dly(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 5)
        mexErrMsgIdAndTxt("ntm:arg", "usage: ntm_mpc_mex('run_dly', x0, k_sim, est, dly[, cfg[, d0[, xhat0[, uq0]]]])");
    const ntm_estimator e = read_est(prhs[3]);
    const ntm_delay d = read_dly(prhs[4]);
    const ntm_config c = read_cfg(nrhs > 5 ? prhs[5] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    const double* x0 = in_matrix(prhs[1], 2, B, "x0");
    const double* d0 = opt_matrix(nrhs, prhs, 6, B, "d0");
    const double* h0 = opt_matrix(nrhs, prhs, 7, B, "xhat0");
    const double* q0 = NULL;
    if (nrhs > 8 && !(mxIsDouble(prhs[8]) && mxGetNumberOfElements(prhs[8]) == 0))
        q0 = in_matrix(prhs[8], (size_t)d.steps, B, "uq0");
    const int k = in_ksim_run(prhs[2]);
    const loop_out o = new_loop_out(k, N, B, 1, 1, 1);
    check(ntm_mpc_run_dly(ctx(), &p, &c, &e, &d, (int64_t)B, k, x0, d0, h0, q0, D(o.xk), D(o.uk), D(o.Uk), D(o.wp),
                          D(o.dk), D(o.xhk), D(o.yk), D(o.uak), D(o.xpk), I(o.fl), I(o.it)),
          "ntm_mpc_run_dly");
    mxArray* outs[11] = {o.xk, o.uk, o.Uk, o.wp, o.fl, o.it, o.dk, o.xhk, o.yk, o.uak, o.xpk};
    put_outs(nlhs, plhs, outs, 11);
}

/* 'run_dly' from a carried state (ntm_mpc_run_dly_from): the state is outputs 12 to 18 */
static void do_run_dly_from(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 11)
        mexErrMsgIdAndTxt(
            "ntm:arg",
            "usage: ntm_mpc_mex('run_dly_from', x, rho, Uold, ws, d_hat, x_hat, u_queue, k_sim, est, dly[, cfg])");
    const ntm_estimator e = read_est(prhs[9]);
    const ntm_delay d = read_dly(prhs[10]);
    const ntm_config c = read_cfg(nrhs > 11 ? prhs[11] : NULL);
    ntm_physics p;
    ntm_physics_default(&p);
    const size_t B = mxGetN(prhs[1]), N = (size_t)c.N;
    in_matrix(prhs[1], 2, B, "x");
    in_matrix(prhs[2], 3 * N, B, "rho");
    in_matrix(prhs[3], N, B, "Uold");
    in_ws(prhs[4], N, B);
    in_matrix(prhs[5], 2, B, "d_hat");
    in_matrix(prhs[6], 2, B, "x_hat");
    in_queue(prhs[7], (size_t)d.steps, B, "u_queue");
    const int k = in_ksim(prhs[8]);
    mxArray* x = mxDuplicateArray(prhs[1]);
    mxArray* rho = mxDuplicateArray(prhs[2]);
    mxArray* uold = mxDuplicateArray(prhs[3]);
    mxArray* ws = mxDuplicateArray(prhs[4]);
    mxArray* dh = mxDuplicateArray(prhs[5]);
    mxArray* xh = mxDuplicateArray(prhs[6]);
    mxArray* uq = d.steps ? mxDuplicateArray(prhs[7]) : mxCreateDoubleMatrix(0, B, mxREAL);
    const loop_out o = new_loop_out(k, N, B, 1, 1, 1);
    check(ntm_mpc_run_dly_from(ctx(), &p, &c, &e, &d, (int64_t)B, k, D(x), D(rho), D(uold), I(ws), D(dh), D(xh),
                               d.steps ? D(uq) : NULL, D(o.xk), D(o.uk), D(o.Uk), D(o.wp), D(o.dk), D(o.xhk), D(o.yk),
                               D(o.uak), D(o.xpk), I(o.fl), I(o.it)),
          "ntm_mpc_run_dly_from");
    mxArray* outs[18] = {o.xk, o.uk,  o.Uk, o.wp, o.fl,  o.it, o.dk, o.xhk, o.yk,
                         o.uak, o.xpk, x,   rho,  uold, ws,   dh,   xh,    uq};
    put_outs(nlhs, plhs, outs, 18);
}

static void do_scenarios(int nrhs, const mxArray* prhs[]) {
    if (nrhs < 2 || (mxIsDouble(prhs[1]) && mxGetNumberOfElements(prhs[1]) == 0)) {
        check(ntm_ctx_set_scenarios(ctx(), NULL), "ntm_ctx_set_scenarios");
        return;
    }
    const mxArray* s = prhs[1];
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("ntm:arg", "gen must be a struct or []");
    ntm_scenario_gen g;
    memset(&g, 0, sizeof g);
    g.seed = (uint64_t)scalar_field(s, "seed", 20241220);
    g.first_id = (int64_t)scalar_field(s, "first_id", 0);
    g.k0 = (int32_t)scalar_field(s, "k0", 0);
    g.sigma_w = scalar_field(s, "sigma_w", 0.0);
    g.sigma_omega = scalar_field(s, "sigma_omega", 0.0);
    g.jbs_spread = scalar_field(s, "jbs_spread", 0.0);
    g.wdep_spread = scalar_field(s, "wdep_spread", 0.0);
    check(ntm_ctx_set_scenarios(ctx(), &g), "ntm_ctx_set_scenarios");
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 1 || !mxIsChar(prhs[0]))
        mexErrMsgIdAndTxt("ntm:arg", "first argument: 'init', 'step', 'run', 'scenarios' or 'close'");
    char cmd[16];
    mxGetString(prhs[0], cmd, sizeof cmd);
    if (!strcmp(cmd, "step")) do_step(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "init")) do_init(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run")) do_run(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "step_obs")) do_step_obs(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run_obs")) do_run_obs(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "step_est")) do_step_est(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run_est")) do_run_est(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run_from")) do_run_from(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run_est_from")) do_run_est_from(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "step_dly")) do_step_dly(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run_dly")) do_run_dly(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "run_dly_from")) do_run_dly_from(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "scenarios")) do_scenarios(nrhs, prhs);
    else if (!strcmp(cmd, "close")) release();
    else mexErrMsgIdAndTxt("ntm:arg", "unknown command '%s'", cmd);
}
