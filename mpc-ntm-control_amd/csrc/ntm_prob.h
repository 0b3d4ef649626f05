// ntm_prob.h — the launch-constant problem description (Coef, Gen, Prob) and the
// counter-based scenario generator.  Host and device code: the library's host-side
// sampler (ntm_scenario_sample) runs the generator the kernels run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ntm {

// ---------------------------------------------------------------------------
// launch-constant problem description (derived on the host, see ntm_capi.hip)
// ---------------------------------------------------------------------------
struct Coef {
    double a11c;    // (4/3)(kappa rs/(0.82 tau_r)) Ts           A.m:2
    double za3;     // zeta * a^3 (D19, divides rho2*Ts)         A.m:2
    double a22;     // 1 - Ts/tau_E                              A.m:2
    double bc;      // kappa Ts eta_CD / w_dep                   B.m:2
    double C1, C2;  // NTM_MPC_Sim.m:37
    double wmarg2;  // w_marg^2                                  rho1.m:2
    double wdep;    // w_dep                                     rho3.m:2
    double Ts;
    int rho1_sq;    // D18 switch
};

// Scenario generator (ntm_ctx_set_scenarios): per-scenario plasma parameters
// and per-step plant disturbances, counter-based on (seed, global scenario id,
// time index), so any sharding or batching reproduces the same realisations.
struct Gen {
    uint64_t seed;
    int64_t first_id;   // global id of the launch's scenario 0
    int k0;             // time index of the launch's first plant step
    int dist_on;        // sigma_w or sigma_omega non-zero
    int phys_on;        // a parameter spread non-zero
    double sw, so;      // disturbance standard deviations (w [m], omega [rad/s])
    double sj, sd;      // j_BS / w_dep spreads
    // host-computed pieces of NTM_MPC_Sim.m:24,37 and B.m:2 the per-scenario
    // C1 and b coefficient are rebuilt from (same expression order as make_prob)
    double kTs, wsat, den, jbs, kte, wdep;
};

struct Prob {
    Coef k;
    int N, i_sim, mode, flags;
    double xmin[2], xmax[2], umin, umax, Q[4], r[2], eps;
    double du;        // input-rate bound (NTM_MODE_FULL_DU)
    int32_t* stats;  // optional per-scenario counters (4 x B, SoA): QP solves,
                      // GI iterations, final active rows, general (state) active rows
    Gen g;
    double* far;      // far workspace (HBM, far_doubles(N) per scenario) of the kernels
                      // whose WS keeps J/R out of LDS (ws_far); null otherwise
    double Ru;        // input weight (ABI v5): G = 2 Gamma' Om Gamma + 2 Ru I; read by the
                      // generic (NN = 0) kernels only, the host sends Ru != 0 there (ru_on);
                      // last, so the specialised kernels' argument layout is unchanged
};


// ---------------------------------------------------------------------------
// Counter-based scenario generator (host and device share this code, so the
// library's host-side sampler ntm_scenario_sample returns the device's values)
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// uniform [0, 1) from (seed, global scenario id, time index k, channel ch < 256)
__host__ __device__ __forceinline__ double gen_u01(uint64_t seed, int64_t sid, uint32_t k, uint32_t ch) {
    uint64_t h = splitmix64(seed ^ 0xD1B54A32D192ED03ull);
    h = splitmix64(h ^ (uint64_t)sid);
    h = splitmix64(h ^ (((uint64_t)k << 8) | ch));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}
// unit-variance, zero-mean Irwin-Hall(4) sample (bounded at +-2 sqrt(3)); only
// + and * so host and device agree bit for bit.  Channel c uses sub-channels 4c..4c+3.
__host__ __device__ __forceinline__ double gen_normal(uint64_t seed, int64_t sid, uint32_t k, uint32_t c) {
    double s = gen_u01(seed, sid, k, 4 * c);
    s = s + gen_u01(seed, sid, k, 4 * c + 1);
    s = s + gen_u01(seed, sid, k, 4 * c + 2);
    s = s + gen_u01(seed, sid, k, 4 * c + 3);
    return (s - 2.0) * 1.7320508075688772;
}
constexpr uint32_t kGenParamK = 0xFFFFFFFFu;   // time index of the per-scenario parameters
// per-scenario factor 1 + spread (2u - 1) of parameter channel c (0 j_BS, 1 w_dep)
// (an explicit fused multiply-add: compilers may or may not contract 1 + a b, so the
// generator fixes the rounding itself and every implementation agrees bit for bit)
__host__ __device__ __forceinline__ double gen_factor(uint64_t seed, int64_t sid, uint32_t c, double spread) {
    return fma(spread, 2.0 * gen_u01(seed, sid, kGenParamK, c) - 1.0, 1.0);
}
// scenario sid's plasma (j_BS, w_dep) into the coefficients that depend on them:
// C1 (NTM_MPC_Sim.m:37), the B.m:2 gain and rho3's w_dep (rho3.m:2)
__host__ __device__ __forceinline__ void gen_apply_physics(Prob& p, int64_t sid) {
    const Gen& g = p.g;
    const double jbs = g.jbs * gen_factor(g.seed, sid, 0, g.sj);
    const double wdep = g.wdep * gen_factor(g.seed, sid, 1, g.sd);
    p.k.C1 = -4.0 / 3.0 * (g.kTs * jbs * g.wsat) / g.den;
    p.k.bc = g.kte / wdep;
    p.k.wdep = wdep;
}

}  // namespace ntm
