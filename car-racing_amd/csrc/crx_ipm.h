// crx_ipm.h -- the interior-point rules that crx_solve_kernel (crx_kernels.hip), crx_lmpc_kernel (crx_lmpc.hip) and crx_path_kernel /
// crx_path_masked_kernel (crx_path_qp.h) share, each stated once.  IPOPT's rules on IPOPT's defaults (the reference runs IPOPT untouched);
// oracle/ keeps its own independent statement of them.
//
// Scalars in, scalars out: no LDS, no lane operations, no loops over rows, no structs.  Inputs go by value (the optimiser sees a
// forceinline function on its own before it is inlined: with `const crx_ipm_opts&` the callers' code changes); ipm_theta_bounds()
// alone hands its two results back through references, which its two callers' code takes unchanged.  How a kernel walks its rows,
// reduces over lanes and stores its filter is the kernel's.  A site goes through a function here only where (a) the kernels'
// arithmetic was operation for operation the same and (b) the kernel's machine code stayed bit for bit what it was
// (tools/kernel_diff.py).  Every function here has a caller; a rule that no kernel can take through a function is stated in the
// table at the end, with every site that writes it out.
//
// Floating-point contraction: every including unit includes this header at its head, in the compiler's default state (hipcc:
// contraction on), so the multiply-adds of ipm_sufficient_decrease(), ipm_filter_phi() and ipm_tau() may fuse exactly as the
// written-out copies did.  No unit under `#pragma clang fp contract(off)` (crx_lmpcprep.hip) includes it.
#ifndef CRX_IPM_H
#define CRX_IPM_H
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/crx.h"

// ---- constants (IPOPT's names) -------------------------------------------------------------------------------------------------
// The backtracking stops at alpha_min ("no acceptable step"; IPOPT's alpha_min plays the same role): below it a step changes nothing
// in double precision relative to the iterate, the trial values differ from the current ones by rounding only, and whether the
// filter happens to accept one of them is noise -- on infeasible problems (slacks collapsed to ~1e-20) that noise used to decide at
// which iteration the solve gave up.
constexpr double IPM_ALPHA_MIN = 1e-10;
constexpr int IPM_MAX_BACKTRACK = 40;      // halvings of the step at most
constexpr double IPM_S_PHI = 2.3;          // switching condition al (-Dphi)^s_phi > delta theta^s_theta, delta = 1
constexpr double IPM_S_THETA = 1.1;
constexpr double IPM_ETA_PHI = 1e-8;       // Armijo
constexpr double IPM_GAMMA_THETA = 1e-5;   // sufficient decrease, and the margins of a filter entry
constexpr double IPM_GAMMA_PHI = 1e-8;
constexpr double IPM_KAPPA_SIGMA = 1e10;   // dual safeguard: nu in [mu / (kappa_sigma t), kappa_sigma mu / t]
constexpr double IPM_EPS = 2.2e-16;        // the machine precision of the Armijo test's rounding allowance, 10 eps |phi0|

// ---- barrier parameter ---------------------------------------------------------------------------------------------------------
// Monotone update: while the error of the barrier problem Emu <= kappa_eps mu and mu is above its floor tol / 10 (ipm_mu_reached),
// mu <- max(tol / 10, min(kappa_mu mu, mu^theta_mu)) (ipm_next_mu) and the caller resets its filter (nf = 0), then looks again with
// the new mu's Emu.  SQRT15: mu^1.5 (the default theta_mu) as mu sqrt(mu) instead of pow().
__device__ __forceinline__ bool ipm_mu_reached(double Emu, double mu, double kappa_eps, double tol) { return Emu <= kappa_eps * mu && mu > tol / 10.0; }
template <bool SQRT15>
__device__ __forceinline__ double ipm_next_mu(double mu, double kappa_mu, double theta_mu, double tol) {
    return fmax(tol / 10.0, fmin(kappa_mu * mu, SQRT15 && theta_mu == 1.5 ? mu * sqrt(mu) : pow(mu, theta_mu)));
}
// fraction to the boundary
__device__ __forceinline__ double ipm_tau(double mu, double tau_min) { return fmax(tau_min, 1.0 - mu); }

// ---- filter line search --------------------------------------------------------------------------------------------------------
// theta_min / theta_max from the constraint violation of the first iterate (of a start, restart or restoration)
__device__ __forceinline__ void ipm_theta_bounds(double theta, double& theta_min, double& theta_max) {
    theta_min = 1e-4 * fmax(1.0, theta);
    theta_max = 1e4 * fmax(1.0, theta);
}
// Acceptance of a trial point (step al: violation thn, merit phin) that has passed the filter, against the current point (theta,
// phi0, directional derivative Dphi).  When theta <= theta_min and the switching condition holds, the Armijo condition decides (an
// f-type step: no filter entry; written out in each kernel, table at the end); otherwise sufficient decrease in either measure (an
// h-type step), which all three kernels take from here.
__device__ __forceinline__ bool ipm_sufficient_decrease(double theta, double thn, double phi0, double phin) {
    return thn <= (1.0 - IPM_GAMMA_THETA) * theta || phin <= phi0 - IPM_GAMMA_PHI * theta;
}
// the filter entry (Fth, Fph) an h-type step leaves behind
__device__ __forceinline__ double ipm_filter_theta(double theta) { return (1.0 - IPM_GAMMA_THETA) * theta; }
__device__ __forceinline__ double ipm_filter_phi(double theta, double phi0) { return phi0 - IPM_GAMMA_PHI * theta; }
// dual safeguard on mu_t = mu / t (the caller's quotient)
__device__ __forceinline__ double ipm_dual_safeguard(double nu, double mu_t) {
    return fmin(fmax(nu, mu_t * (1.0 / IPM_KAPPA_SIGMA)), IPM_KAPPA_SIGMA * mu_t);
}

// ---- inertia correction --------------------------------------------------------------------------------------------------------
// IPOPT's delta_w schedule (Alg. IC) for a Newton system whose factorisation shows the wrong inertia: the first delta_w is 1e-4 on a
// cold start (dw_last == 0: no system of this solve has needed one yet) and a third of the last successful one otherwise, floored at
// 1e-20; every further attempt multiplies it by 100 (cold) or 8 (warm); above IPM_DW_MAX the schedule is exhausted and the solve gives
// up.  How the attempts are run (one sweep at a time, two at a time, inside the sweep function) is the kernel's.
constexpr double IPM_DW_MAX = 1e40;
__device__ __forceinline__ double ipm_dw_first(double dw_last) { return dw_last == 0.0 ? 1e-4 : fmax(1e-20, dw_last / 3.0); }
__device__ __forceinline__ double ipm_dw_grow(double dw, double dw_last) { return dw * (dw_last == 0.0 ? 100.0 : 8.0); }

// ---- Differences between the kernels that are NOT shared, and why each stays -----------------------------------------------------
// "code changes" = with this one site alone routed through a function of this header (by-value scalars, the written-out expression
// as its body), the kernel's machine code is no longer bit for bit what it was (tools/kernel_diff.py `differs (text)`), although
// the arithmetic is the same; the site uses the named constants and carries a comment "crx_ipm.h, table".  A later change that is
// allowed to move the code can route these on purpose.  Lines as of this header's last edit; the kernel and the comment find them.
//
// Termination, IPOPT's COMPLETE test (OptimalityErrorConvergenceCheck), written out at four sites and in no function:
//     E0 <= tol  &&  dual_inf <= dual_inf_tol (1)  &&  constr_viol <= constr_viol_tol (1e-4)  &&  compl_inf <= compl_inf_tol (1e-4)
// with E0 the scaled error and the other three unscaled (no s_d / s_c, rows in the reference's units).  The second half binds on
// crash states: multipliers of 1e7..1e9 make s_d 1e4..1e7 and the scaled complementarity passes at mu = 1e-4 already.
// Armijo condition of an f-type step, written out at three sites and in no function:
//     phin <= phi0 + IPM_ETA_PHI al Dphi + 10 IPM_EPS |phi0|
//
//   rule                   kernel (file:line)                                  why it stays
//   termination test       crx_solve_kernel, Mehrotra (crx_kernels.hip:2263)   code changes in 5 of 39 solver instantiations
//                          crx_solve_kernel, NLP (crx_kernels.hip:2430-2446)   code changes in 32 of 39 (the E0 test guards the lazy row pass for vu)
//                          crx_lmpc_kernel (crx_lmpc.hip:529)                  code changes in all six instantiations
//                          crx_path_kernel (crx_path_qp.h:71)                  code changes (the products e_d * sd, e_c * sd are evaluated lazily there)
//   barrier update         crx_lmpc_kernel (crx_lmpc.hip:560-561)              code changes in <12,0,44,*>; same arithmetic as ipm_mu_reached / ipm_next_mu<true>
//   mu^theta_mu            crx_path_kernel (crx_path_qp.h:76)                  DIFFERENT ARITHMETIC: ipm_next_mu<false>, pow() for every theta_mu; the other
//                                                                              two kernels mu sqrt(mu) at 1.5
//   theta_min / theta_max  crx_lmpc_kernel (crx_lmpc.hip:801-804)              code changes in all six instantiations
//   switching condition    crx_solve_kernel (crx_kernels.hip:2644-2648, :2699) DIFFERENT ARITHMETIC, three forms: log2 domain with the al-independent part
//                          crx_lmpc_kernel (crx_lmpc.hip:826)                  hoisted (solver), log2 domain inline (learning MPC), two pow() (path).  The
//                          crx_path_kernel (crx_path_qp.h:131)                 exponents are IPM_S_PHI / IPM_S_THETA in all three.
//   Armijo condition       crx_solve_kernel (crx_kernels.hip:2700)             code changes in 32 of 39 solver instantiations
//                          crx_lmpc_kernel (crx_lmpc.hip:828)                  code changes in all six instantiations
//                          crx_path_kernel (crx_path_qp.h:133)                 code changes
//   dual safeguard         crx_path_kernel (crx_path_qp.h:150-151)             DIFFERENT ARITHMETIC: mu / (kappa_sigma t) and kappa_sigma mu / t; the other
//                                                                              two kernels clamp against mu_t = mu * rcp(t): ipm_dual_safeguard
// Shared by all three kernels: tau, sufficient decrease, the filter entry, alpha_min and the backtrack count, every constant.  By the
// solver and the path kernel: the barrier update, theta_min / theta_max.  By the solver and the learning-MPC kernel: the dual
// safeguard.  By the four sites of the solver that walk it (the other two kernels factorise convex QPs and have none): the delta_w
// schedule of the inertia correction, ipm_dw_first / ipm_dw_grow / IPM_DW_MAX.

#endif
