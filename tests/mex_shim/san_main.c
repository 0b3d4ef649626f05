/*
 * san_main.c — TEST-ONLY stand-alone driver of the MEX gateway's argument-error paths, for
 * a sanitizer run on the CPU (no GPU, no Python: every call here fails before the library
 * is asked for a context).  From this directory:
 *
 *   gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wextra -Werror \
 *       -I . -I ../../include ../../integration/matlab/ntm_mpc_mex.c mex_shim.c san_main.c \
 *       -L ../../mpc-ntm-control_amd/lib -lntm_mpc -Wl,-rpath,$PWD/../../mpc-ntm-control_amd/lib -o mex_san
 *   ASAN_OPTIONS=detect_leaks=0 ./mex_san
 *
 * (detect_leaks=0: an error leaves the gateway by longjmp in the shim, so arrays made before
 * it stay allocated; MATLAB frees them itself.)  For each of the twelve commands: too few
 * arguments, every array argument in turn with a row too many and with the wrong class, a
 * non-struct where a struct belongs, a bad k_sim; each must raise ntm:arg or ntm:cfg.  Prints
 * the number of errors raised; exit 1 if a call returned or raised something else.
 */
#include <stdio.h>
#include <string.h>

#include "mex.h"

mxArray* t_double(size_t m, size_t n, const double* d);
mxArray* t_int32(size_t m, size_t n, const int32_t* d);
mxArray* t_char(const char* s);
mxArray* t_struct(void);
void t_struct_set(mxArray* s, const char* name, mxArray* v);
void t_free(mxArray* a);
const char* t_err_id(void);
const char* t_err_msg(void);
int t_call(int nlhs, mxArray** plhs, int nrhs, mxArray** prhs);

enum { B = 3, N = 4, STEPS = 3, MAXA = 13 };

/* one argument by kind: x/d (2-by-B), r (3N), u (N), q (STEPS), w (int32 2(N+1)), k (scalar 2),
 * c (cfg struct), o / e / y (obs, est, dly structs); rows + extra, cls: 0 as is, 1 the other class */
static mxArray* make_arg(char kind, int extra, int other) {
    size_t rows = 0;
    mxArray* s;
    mxArray* v;
    switch (kind) {
    case 'x': rows = 2; break;
    case 'r': rows = 3 * N; break;
    case 'u': rows = N; break;
    case 'q': rows = STEPS; break;
    case 'w': rows = 2 * (N + 1); break;
    case 'k': return extra ? t_double(1, 1, (double[]){-1.0}) : other ? t_struct() : t_double(1, 1, (double[]){2.0});
    default:
        if (other) return t_double(1, 1, NULL);
        s = t_struct();
        v = t_double(1, 1, (double[]){kind == 'c' ? (double)N : kind == 'y' ? (double)(extra ? 9 : STEPS) : 1.0});
        t_struct_set(s, kind == 'c' ? "N" : kind == 'y' ? "steps" : "nominal_model", v);
        return s;
    }
    return ((kind == 'w') != (other != 0)) ? t_int32(rows + (size_t)extra, B, NULL) : t_double(rows + (size_t)extra, B, NULL);
}

static int n_raised = 0, n_bad = 0;

/* call cmd with the first n kinds of sig; argument `at` (or none: -1) made wrong */
static void expect_error(const char* cmd, const char* sig, int n, int at, int extra, int other) {
    mxArray* prhs[MAXA + 1];
    mxArray* plhs[20];
    prhs[0] = t_char(cmd);
    for (int i = 0; i < n; ++i) prhs[i + 1] = make_arg(sig[i], i == at ? extra : 0, i == at ? other : 0);
    const int rc = t_call(18, plhs, n + 1, prhs);
    if (rc && (!strcmp(t_err_id(), "ntm:arg") || !strcmp(t_err_id(), "ntm:cfg"))) {
        ++n_raised;
    } else {
        ++n_bad;
        fprintf(stderr, "%s (%d arguments, %d wrong): %s %s\n", cmd, n, at, rc ? t_err_id() : "returned", t_err_msg());
    }
    for (int i = 0; i <= n; ++i) t_free(prhs[i]);
}

int main(void) {
    /* command, its full argument kinds, the number of required ones */
    static const struct { const char *cmd, *sig; int need; } cmds[] = {
        {"step", "xrucw", 3},          {"init", "xc", 1},           {"run", "xkc", 2},
        {"step_obs", "xruxocw", 5},    {"run_obs", "xkocx", 3},     {"step_est", "xruxxecw", 6},
        {"run_est", "xkecxx", 3},      {"run_from", "xruwkc", 5},   {"run_est_from", "xruwxxkec", 8},
        {"step_dly", "xruxxqeycw", 8}, {"run_dly", "xkeycxxq", 4},  {"run_dly_from", "xruwxxqkeyc", 10},
    };
    for (size_t c = 0; c < sizeof cmds / sizeof cmds[0]; ++c) {
        const int n = (int)strlen(cmds[c].sig);
        for (int few = 0; few < cmds[c].need; ++few) expect_error(cmds[c].cmd, cmds[c].sig, few, -1, 0, 0);
        for (int at = 0; at < n; ++at) {
            const char kind = cmds[c].sig[at];
            /* 'run*' reads its k_sim with mxGetScalar: only a value below 1 is an error there */
            const int run_k = kind == 'k' && !strstr(cmds[c].cmd, "_from");
            if (strchr("xruqwy", kind)) expect_error(cmds[c].cmd, cmds[c].sig, n, at, 1, 0);
            if (kind == 'k') expect_error(cmds[c].cmd, cmds[c].sig, n, at, 1, 0);
            if (!run_k) expect_error(cmds[c].cmd, cmds[c].sig, n, at, 0, 1);
        }
    }
    expect_error("frobnicate", "", 0, -1, 0, 0);
    printf("%d argument errors raised, %d calls went wrong\n", n_raised, n_bad);
    return n_bad != 0;
}
