// k_pnp_mse.hip — min-MSE PnP: the second IPnpAlgorithm of the reference (MinMseTracker).
//
// Replaces MinMseTracker::solvePnp (reference ceres_reprojection_error_pnp.cpp:18-110): a Ceres Levenberg-Marquardt
// solve over x = (r, t) (angle-axis r, translation t) of
//     cost(x) = 1/2 sum_i |obs_i - proj(AngleAxisRotatePoint(r, P_i) + t)|^2,   proj(X) = (fx X/Z + cx, fy Y/Z + cy)
// with no loss function (mslam_hip_set_pnp_mse_loss sets one, an extension: k_pnp_min_mse_loss below, cost 1/2 sum rho, rho' on
// every product of a point's share of the sums), started from the caller's pose, gradient / function /
// parameter tolerance 1e-8 (:88-90) and every other option at Solver::Options' default.  The minimiser is Ceres 2.2's published trust-region loop
// (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc, trust_region_step_evaluator.cc, solver.cc), written out
// here for a wave that keeps one problem in registers; the defaults, the termination codes and the butterfly sum are
// trust_region.hpp's, which holds the same loop as control-block kernels for k_ba.hip and k_posegraph.hip.  The
// SAME / DEVIATES table is in include/mslam_hip.h, the walk-through in DESIGN.md.  Parity with a Ceres build is UNPINNED
// (none exists in this image); tests/mse_pnp_ref.py restates the same algorithm in numpy and the tests pin both against
// each other and against ground truth.
//
// Layout: one wave64 per problem, kMseWaves problems per workgroup.  The lanes stride over the points; each evaluates
// the residuals and their derivatives by forward-mode dual numbers (what ceres::AutoDiffCostFunction does) and
// accumulates the 21 upper-triangle entries of J^T J, the 6 of J^T f and the cost.  A fixed-order __shfl_xor butterfly
// reduces them: IEEE addition is commutative, so every lane ends with bit-identical totals, and every lane then runs the
// 6x6 solve and the trust-region bookkeeping redundantly in registers.  No LDS, no barriers, uniform control flow.
// Each trust-region iteration is one sweep over the points at the candidate point (value and derivatives together:
// an accepted candidate needs its Jacobian next, a rejected one discards it).  All arithmetic is f64.
#include "trust_region.hpp"

#include <algorithm>

namespace mslam
{

constexpr int kMseWaves = 4; // problems (waves) per workgroup
constexpr int kMseThreads = 64 * kMseWaves;

// what differs from trust_region.hpp's Solver::Options defaults: max_num_iterations, and the three tolerances of the call
// site (ceres_reprojection_error_pnp.cpp:88-90)
constexpr int kMseMaxIterations = 50;
constexpr double kMseGradientTol = 1e-8, kMseFunctionTol = 1e-8, kMseParameterTol = 1e-8;

struct MseArgs
{
    const double* obj; // [n_problems][capacity][3]
    const double* img; // [n_problems][capacity][2]
    const int32_t* n;  // [n_problems]
    int n_problems, capacity;
    double fx, fy, cx, cy;
    double* pose; // [n_problems][6] (r, t): start in, result out
    double* info; // [n_problems][4]: termination, iterations, initial cost, final cost
};

// ceres::Jet<double, N> (jet.h): value a, derivatives v; the operations below are the ones AngleAxisRotatePoint and the
// functor use, each with the formula jet.h evaluates
template <int N>
struct Jet
{
    double a;
    double v[N];
};

template <int N>
__device__ __forceinline__ Jet<N> operator+(const Jet<N>& f, const Jet<N>& g)
{
    Jet<N> r;
    r.a = f.a + g.a;
    for(int k = 0; k < N; ++k)
        r.v[k] = f.v[k] + g.v[k];
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator-(const Jet<N>& f, const Jet<N>& g)
{
    Jet<N> r;
    r.a = f.a - g.a;
    for(int k = 0; k < N; ++k)
        r.v[k] = f.v[k] - g.v[k];
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(const Jet<N>& f, const Jet<N>& g)
{
    Jet<N> r;
    r.a = f.a * g.a;
    for(int k = 0; k < N; ++k)
        r.v[k] = f.a * g.v[k] + f.v[k] * g.a;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator*(const Jet<N>& f, double s)
{
    Jet<N> r;
    r.a = f.a * s;
    for(int k = 0; k < N; ++k)
        r.v[k] = f.v[k] * s;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> operator/(const Jet<N>& f, const Jet<N>& g)
{
    const double g_a_inverse = 1.0 / g.a;
    const double f_a_by_g_a = f.a * g_a_inverse;
    Jet<N> r;
    r.a = f_a_by_g_a;
    for(int k = 0; k < N; ++k)
        r.v[k] = (f.v[k] - f_a_by_g_a * g.v[k]) * g_a_inverse;
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> scalar_minus(double s, const Jet<N>& g)
{
    Jet<N> r;
    r.a = s - g.a;
    for(int k = 0; k < N; ++k)
        r.v[k] = -g.v[k];
    return r;
}
template <int N>
__device__ __forceinline__ Jet<N> jsqrt(const Jet<N>& f)
{
    const double s = sqrt(f.a);
    const double two_a_inverse = 1.0 / (2.0 * s);
    Jet<N> r;
    r.a = s;
    for(int k = 0; k < N; ++k)
        r.v[k] = f.v[k] * two_a_inverse;
    return r;
}
template <int N>
__device__ __forceinline__ void jsincos(const Jet<N>& f, Jet<N>& s, Jet<N>& c)
{
    const double sa = sin(f.a), ca = cos(f.a);
    s.a = sa;
    c.a = ca;
    for(int k = 0; k < N; ++k)
    {
        s.v[k] = ca * f.v[k];
        c.v[k] = -sa * f.v[k];
    }
}

// residuals (u - xp, v - yp) of one point and their derivatives d/d(r, t).  The rotation depends on r alone, so it runs on
// 3-slot jets; the translation's slots of the rotated point are exactly 0 in Ceres's 6-slot jets, and adding t (seeded
// e_3..e_5) makes them 1 / 0, which is what the 6-slot jets below start from.
__device__ __forceinline__ void mse_residual(const double x[6], const double P[3], double u, double v, double fx, double fy,
                                             double cx, double cy, double res[2], double J[2][6])
{
    Jet<3> r[3];
    for(int i = 0; i < 3; ++i)
    {
        r[i].a = x[i];
        for(int k = 0; k < 3; ++k)
            r[i].v[k] = i == k ? 1.0 : 0.0;
    }
    Jet<3> rot[3];
    // ceres::AngleAxisRotatePoint (rotation.h)
    const Jet<3> theta2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    if(theta2.a > DBL_EPSILON)
    {
        const Jet<3> theta = jsqrt(theta2);
        Jet<3> sintheta, costheta;
        jsincos(theta, sintheta, costheta);
        const Jet<3> one = {1.0, {0.0, 0.0, 0.0}};
        const Jet<3> theta_inverse = one / theta; // T(1.0) / theta: a jet over a jet
        const Jet<3> w[3] = {r[0] * theta_inverse, r[1] * theta_inverse, r[2] * theta_inverse};
        const Jet<3> w_cross_pt[3] = {w[1] * P[2] - w[2] * P[1], w[2] * P[0] - w[0] * P[2], w[0] * P[1] - w[1] * P[0]};
        const Jet<3> tmp = (w[0] * P[0] + w[1] * P[1] + w[2] * P[2]) * scalar_minus(1.0, costheta);
        for(int i = 0; i < 3; ++i)
        {
            // pt[i] * costheta + w_cross_pt[i] * sintheta + w[i] * tmp  (a constant times a jet: jet.h's s * f)
            rot[i] = costheta * P[i] + w_cross_pt[i] * sintheta + w[i] * tmp;
        }
    }
    else
    {
        const Jet<3> w_cross_pt[3] = {r[1] * P[2] - r[2] * P[1], r[2] * P[0] - r[0] * P[2], r[0] * P[1] - r[1] * P[0]};
        for(int i = 0; i < 3; ++i)
        {
            rot[i].a = P[i] + w_cross_pt[i].a;
            for(int k = 0; k < 3; ++k)
                rot[i].v[k] = w_cross_pt[i].v[k];
        }
    }
    Jet<6> pt2[3];
    for(int i = 0; i < 3; ++i)
    {
        pt2[i].a = rot[i].a + x[3 + i];
        for(int k = 0; k < 3; ++k)
            pt2[i].v[k] = rot[i].v[k], pt2[i].v[3 + k] = i == k ? 1.0 : 0.0;
    }
    const Jet<6> xq = pt2[0] / pt2[2], yq = pt2[1] / pt2[2];
    // T(f) * q + T(c), then observed - projected
    res[0] = u - (xq.a * fx + cx);
    res[1] = v - (yq.a * fy + cy);
    for(int k = 0; k < 6; ++k)
    {
        J[0][k] = -(xq.v[k] * fx);
        J[1][k] = -(yq.v[k] * fy);
    }
}

// Sums over the problem's points at x: cost, J^T J (upper triangle, row-major), J^T f.  Every lane returns the same bits.
struct MseSums
{
    double cost;
    double H[21];
    double g[6];
};

// what k_pnp_min_mse_loss's launch carries.  The loss travels in the argument's type (Args below), not as one more parameter
// of mse_sweep and mse_problem: with a further parameter k_pnp_min_mse's registers are numbered anew
struct MseLossArgs : MseArgs
{
    TrLoss loss; // mslam_hip_set_pnp_mse_loss: HUBER or CAUCHY, a in pixels
};

// kLoss (Args = MseLossArgs): with s = res0^2 + res1^2 the lane adds 0.5 rho(s) to the cost and w = rho'(s) times the
// product to each of the 21 + 6 sums.  The sweep keeps no rows that could be scaled by sqrt(w), so the weight goes on the
// products, as in k_ba.hip (DEVIATES in rounding from Ceres's corrector, include/mslam_hip.h)
template <bool kLoss, class Args>
__device__ void mse_sweep(const Args& a, const double* obj, const double* img, int n, int lane, const double x[6], MseSums& S)
{
    S.cost = 0.0;
    for(int k = 0; k < 21; ++k)
        S.H[k] = 0.0;
    for(int k = 0; k < 6; ++k)
        S.g[k] = 0.0;
    for(int i = lane; i < n; i += 64)
    {
        const double P[3] = {obj[(size_t)i * 3], obj[(size_t)i * 3 + 1], obj[(size_t)i * 3 + 2]};
        double res[2], J[2][6];
        mse_residual(x, P, img[(size_t)i * 2], img[(size_t)i * 2 + 1], a.fx, a.fy, a.cx, a.cy, res, J);
        if constexpr(kLoss)
        {
            double rho, w;
            tr_loss(a.loss.kind, a.loss.scale, res[0] * res[0] + res[1] * res[1], rho, w);
            S.cost += 0.5 * rho;
            int k = 0;
            for(int r = 0; r < 6; ++r)
            {
                for(int c = r; c < 6; ++c)
                    S.H[k++] += w * (J[0][r] * J[0][c] + J[1][r] * J[1][c]);
                S.g[r] += w * (J[0][r] * res[0] + J[1][r] * res[1]);
            }
        }
        else
        {
            S.cost += 0.5 * (res[0] * res[0] + res[1] * res[1]);
            int k = 0;
            for(int r = 0; r < 6; ++r)
            {
                for(int c = r; c < 6; ++c)
                    S.H[k++] += J[0][r] * J[0][c] + J[1][r] * J[1][c];
                S.g[r] += J[0][r] * res[0] + J[1][r] * res[1];
            }
        }
    }
    S.cost = wave_sum(S.cost);
    for(int k = 0; k < 21; ++k)
        S.H[k] = wave_sum(S.H[k]);
    for(int k = 0; k < 6; ++k)
        S.g[k] = wave_sum(S.g[k]);
}

// the sums are usable as an evaluation with a Jacobian.  ResidualBlock::Evaluate rejects non-finite residuals or Jacobian
// entries, and any such entry makes the cost or a diagonal entry of J^T J (a sum of squares) non-finite.  The converse
// does not hold: a finite entry above sqrt(DBL_MAX), about 1.3e154, squares to infinity, so such an evaluation fails here
// and would pass in Ceres (DEVIATES `evaluation valid` in include/mslam_hip.h; no physical scene reaches such values)
__device__ __forceinline__ bool sums_finite(const MseSums& S)
{
    bool ok = isfinite(S.cost);
    for(int r = 0; r < 6; ++r)
        ok = ok && isfinite(S.H[tri6(r, r)]) && isfinite(S.g[r]);
    return ok;
}

// |x - Plus(x, -g)|_inf (TrustRegionMinimizer::EvaluateGradientAndJacobian)
__device__ __forceinline__ double gradient_max_norm(const double x[6], const double g[6])
{
    double m = 0.0;
    for(int k = 0; k < 6; ++k)
        m = fmax(m, fabs(x[k] - (x[k] + (-g[k]))));
    return m;
}

template <bool kLoss, class Args>
__device__ void mse_problem(const Args& a, int p, int lane)
{
    double* pose = a.pose + (size_t)p * 6;
    double* info = a.info + (size_t)p * 4;
    const int n = a.n[p];
    double x[6];
    for(int k = 0; k < 6; ++k)
        x[k] = pose[k];
    auto finish = [&](int termination, int iterations, double initial_cost, double final_cost, bool write_pose) {
        if(lane == 0)
        {
            if(write_pose)
                for(int k = 0; k < 6; ++k)
                    pose[k] = x[k];
            info[0] = termination, info[1] = iterations, info[2] = initial_cost, info[3] = final_cost;
        }
    };
    if(n < 0 || n > a.capacity)
    {
        finish(kTrFailure, 0, NAN, NAN, false);
        return;
    }
    if(n == 0)
    {
        // solver.cc Minimize(): a reduced program without parameter blocks is CONVERGENCE at cost 0, parameters untouched
        finish(kTrConvergence, 0, 0.0, 0.0, false);
        return;
    }
    const double* obj = a.obj + (size_t)p * a.capacity * 3;
    const double* img = a.img + (size_t)p * a.capacity * 2;

    // iteration 0 (TrustRegionMinimizer::IterationZero)
    MseSums X;
    mse_sweep<kLoss>(a, obj, img, n, lane, x, X);
    const double initial_cost = X.cost;
    if(!sums_finite(X))
    {
        finish(kTrFailure, 0, initial_cost, initial_cost, false);
        return;
    }
    // Jacobi scaling, once, from the Jacobian at the start: 1 / (1 + |J_col|)
    double s[6];
    for(int k = 0; k < 6; ++k)
        s[k] = 1.0 / (1.0 + sqrt(X.H[tri6(k, k)]));
    double gmax = gradient_max_norm(x, X.g);
    double radius = kTrInitialRadius, decrease_factor = 2.0;
    int invalid_steps = 0, iteration = 0;
    bool successful = true;
    for(;;)
    {
        // FinalizeIterationAndCheckIfMinimizerCanContinue
        if(iteration >= kMseMaxIterations)
        {
            finish(kTrNoConvergence, iteration, initial_cost, X.cost, true);
            return;
        }
        if(successful && gmax <= kMseGradientTol)
        {
            finish(kTrConvergence, iteration, initial_cost, X.cost, true);
            return;
        }
        if(radius <= kTrMinRadius)
        {
            finish(kTrConvergence, iteration, initial_cost, X.cost, true);
            return;
        }
        ++iteration;
        successful = false;

        // LevenbergMarquardtStrategy::ComputeStep on the column-scaled Jacobian Js = J S:
        // (Js^T Js + D^2) y = Js^T f, D^2 = clamp(diag(Js^T Js), 1e-6, 1e32) / radius, step = -y
        double A[21], gs[6];
        for(int r = 0; r < 6; ++r)
        {
            gs[r] = s[r] * X.g[r];
            for(int c = r; c < 6; ++c)
                A[tri6(r, c)] = s[r] * X.H[tri6(r, c)] * s[c];
        }
        double Hs_diag[6];
        for(int k = 0; k < 6; ++k)
        {
            Hs_diag[k] = A[tri6(k, k)];
            A[tri6(k, k)] += fmin(fmax(Hs_diag[k], kTrMinDiagonal), kTrMaxDiagonal) / radius;
        }
        // Cholesky A = L L^T in place (lower triangle stored at tri6(c, r)); a non-positive pivot is a linear-solver failure
        bool solved = true;
        double L[21];
        for(int k = 0; k < 21; ++k)
            L[k] = A[k];
        for(int j = 0; j < 6; ++j)
        {
            double d = L[tri6(j, j)];
            for(int k = 0; k < j; ++k)
                d -= L[tri6(k, j)] * L[tri6(k, j)];
            if(!(d > 0.0))
                solved = false;
            d = sqrt(fmax(d, DBL_MIN));
            L[tri6(j, j)] = d;
            for(int i = j + 1; i < 6; ++i)
            {
                double e = L[tri6(j, i)];
                for(int k = 0; k < j; ++k)
                    e -= L[tri6(k, i)] * L[tri6(k, j)];
                L[tri6(j, i)] = e / d;
            }
        }
        double ds[6];
        for(int i = 0; i < 6; ++i)
        {
            double e = gs[i];
            for(int k = 0; k < i; ++k)
                e -= L[tri6(k, i)] * ds[k];
            ds[i] = e / L[tri6(i, i)];
        }
        for(int i = 5; i >= 0; --i)
        {
            double e = ds[i];
            for(int k = i + 1; k < 6; ++k)
                e -= L[tri6(i, k)] * ds[k];
            ds[i] = e / L[tri6(i, i)];
        }
        for(int k = 0; k < 6; ++k)
        {
            ds[k] = -ds[k];
            solved = solved && isfinite(ds[k]);
        }
        // model cost change -(f^T Js ds + |Js ds|^2 / 2) from the normal equations (Js^T Js without the damping)
        double model_cost_change = 0.0;
        if(solved)
        {
            double lin = 0.0, quad = 0.0;
            for(int r = 0; r < 6; ++r)
            {
                lin += gs[r] * ds[r];
                double hr = 0.0;
                for(int c = 0; c < 6; ++c)
                    hr += s[r] * X.H[r <= c ? tri6(r, c) : tri6(c, r)] * s[c] * ds[c];
                quad += ds[r] * hr;
            }
            model_cost_change = -(lin + 0.5 * quad);
        }
        if(!(solved && model_cost_change > 0.0))
        {
            // HandleInvalidStep
            if(++invalid_steps >= kTrMaxInvalidSteps)
            {
                finish(kTrFailure, iteration, initial_cost, X.cost, false);
                return;
            }
            radius /= decrease_factor; // StepIsInvalid = StepRejected(0)
            decrease_factor *= 2.0;
            continue;
        }
        invalid_steps = 0;
        double cand[6];
        for(int k = 0; k < 6; ++k)
            cand[k] = x[k] + ds[k] * s[k]; // delta = step * jacobian_scaling, Plus = x + delta
        MseSums C;
        mse_sweep<kLoss>(a, obj, img, n, lane, cand, C);
        // a candidate that fails to evaluate is a step of infinite cost (ComputeCandidatePointAndEvaluateCost)
        const double cand_cost = isfinite(C.cost) ? C.cost : DBL_MAX;
        // ParameterToleranceReached
        double x_norm2 = 0.0, step_norm2 = 0.0;
        for(int k = 0; k < 6; ++k)
        {
            x_norm2 += x[k] * x[k];
            const double dk = x[k] - cand[k];
            step_norm2 += dk * dk;
        }
        if(sqrt(step_norm2) <= kMseParameterTol * (sqrt(x_norm2) + kMseParameterTol))
        {
            finish(kTrConvergence, iteration, initial_cost, X.cost, true);
            return;
        }
        // FunctionToleranceReached
        if(fabs(X.cost - cand_cost) <= kMseFunctionTol * X.cost)
        {
            finish(kTrConvergence, iteration, initial_cost, X.cost, true);
            return;
        }
        // IsStepSuccessful (monotonic: the step evaluator's reference cost is the current cost)
        const double relative_decrease = cand_cost >= DBL_MAX ? -DBL_MAX : (X.cost - cand_cost) / model_cost_change;
        if(relative_decrease > kTrMinRelativeDecrease)
        {
            // HandleSuccessfulStep: the Jacobian at the new point
            if(!sums_finite(C))
            {
                finish(kTrFailure, iteration, initial_cost, X.cost, false);
                return;
            }
            for(int k = 0; k < 6; ++k)
                x[k] = cand[k];
            X = C;
            gmax = gradient_max_norm(x, X.g);
            successful = true;
            const double q = 2.0 * relative_decrease - 1.0;
            radius = radius / fmax(1.0 / 3.0, 1.0 - q * q * q);
            radius = fmin(kTrMaxRadius, radius);
            decrease_factor = 2.0;
        }
        else
        {
            radius /= decrease_factor;
            decrease_factor *= 2.0;
        }
    }
}

__global__ __launch_bounds__(kMseThreads) void k_pnp_min_mse(MseArgs a)
{
    const int p = blockIdx.x * kMseWaves + (int)(threadIdx.x >> 6);
    if(p >= a.n_problems)
        return;
    mse_problem<false>(a, p, (int)(threadIdx.x & 63));
}

// mslam_hip_set_pnp_mse_loss: the second form, launched only with HUBER or CAUCHY
__global__ __launch_bounds__(kMseThreads) void k_pnp_min_mse_loss(MseLossArgs a)
{
    const int p = blockIdx.x * kMseWaves + (int)(threadIdx.x >> 6);
    if(p >= a.n_problems)
        return;
    mse_problem<true>(a, p, (int)(threadIdx.x & 63));
}

// the context's loss; NONE: the launch of before the setting existed
static void launch_min_mse(const mslam_hip_ctx* c, const MseArgs& a, hipStream_t stream)
{
    const dim3 grid((a.n_problems + kMseWaves - 1) / kMseWaves);
    if(c->mse_loss_kind != MSLAM_HIP_BA_LOSS_NONE)
    {
        MseLossArgs la{};
        static_cast<MseArgs&>(la) = a;
        la.loss = TrLoss{c->mse_loss_kind, c->mse_loss_scale};
        hipLaunchKernelGGL(k_pnp_min_mse_loss, grid, dim3(kMseThreads), 0, stream, la);
    }
    else
        hipLaunchKernelGGL(k_pnp_min_mse, grid, dim3(kMseThreads), 0, stream, a);
}

} // namespace mslam

using namespace mslam;

extern "C" int mslam_hip_pnp_min_mse(mslam_hip_ctx* c, const double* object_points, const double* image_points, int n,
                                     double fx, double fy, double cx, double cy, double* rvec, double* tvec,
                                     int* termination, int* iterations, double* final_cost)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    auto fail = [&](int code, const char* msg) {
        c->err = msg;
        return code;
    };
    if(n < 0 || (n > 0 && (!object_points || !image_points)) || !rvec || !tvec)
        return fail(MSLAM_HIP_E_INVALID, "pnp_min_mse: bad argument (n >= 0, point and pose pointers)");
    if(n > (1 << 26))
        return fail(MSLAM_HIP_E_INVALID, "pnp_min_mse: too many points");
    hipError_t e = hipSetDevice(c->p.device);
#define PCHK(call)                                                                                                     \
    if(e == hipSuccess)                                                                                                \
    e = (call)
    // one device block: [obj n*3 | img n*2 | pose 6 | info 4 | n (int32 in an 8-byte slot)], grown on demand, so the call
    // is one upload, one launch (the batched kernel with one problem of capacity n) and one download
    const size_t words = (size_t)n * 5 + 11;
    if(words > c->d_mse1.size())
        PCHK(grow(c->d_mse1, std::max<size_t>(words, 5 * 1024 + 11), c->stream));
    std::vector<double> stage(words);
    if(n > 0)
    {
        std::memcpy(stage.data(), object_points, (size_t)n * 24);
        std::memcpy(stage.data() + (size_t)n * 3, image_points, (size_t)n * 16);
    }
    double* pose = stage.data() + (size_t)n * 5;
    pose[0] = rvec[0], pose[1] = rvec[1], pose[2] = rvec[2], pose[3] = tvec[0], pose[4] = tvec[1], pose[5] = tvec[2];
    const int32_t n32 = n;
    std::memcpy(stage.data() + (size_t)n * 5 + 10, &n32, 4);
    double* d = c->d_mse1;
    PCHK(hipMemcpyAsync(d, stage.data(), words * 8, hipMemcpyHostToDevice, c->stream));
    MseArgs a{};
    a.obj = d, a.img = d + (size_t)n * 3;
    a.n = reinterpret_cast<const int32_t*>(d + (size_t)n * 5 + 10);
    a.n_problems = 1, a.capacity = n;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.pose = d + (size_t)n * 5, a.info = d + (size_t)n * 5 + 6;
    if(e == hipSuccess)
        launch_min_mse(c, a, c->stream);
    PCHK(hipGetLastError());
    double out[10];
    PCHK(hipMemcpyAsync(out, a.pose, sizeof(out), hipMemcpyDeviceToHost, c->stream));
    PCHK(hipStreamSynchronize(c->stream));
#undef PCHK
    if(e != hipSuccess)
    {
        c->err = std::string("pnp_min_mse: ") + hipGetErrorString(e);
        return MSLAM_HIP_E_RUNTIME;
    }
    const int term = (int)out[6];
    if(termination)
        *termination = term;
    if(iterations)
        *iterations = (int)out[7];
    if(final_cost)
        *final_cost = out[9];
    if(term == kTrFailure) // Summary::IsSolutionUsable() == false
        return fail(MSLAM_HIP_E_NO_MODEL, "pnp_min_mse: the minimiser ended in FAILURE (non-finite cost or Jacobian, or "
                                          "5 invalid steps in a row)");
    rvec[0] = out[0], rvec[1] = out[1], rvec[2] = out[2];
    tvec[0] = out[3], tvec[1] = out[4], tvec[2] = out[5];
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_pnp_min_mse_batch_dev(mslam_hip_ctx* c, const double* d_object, const double* d_image,
                                               const int32_t* d_n, int n_problems, int capacity, double fx, double fy,
                                               double cx, double cy, double* d_pose, double* d_info)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(n_problems < 0 || capacity < 0 || (n_problems > 0 && (!d_n || !d_pose || !d_info)) ||
       (n_problems > 0 && capacity > 0 && (!d_object || !d_image)))
    {
        c->err = "pnp_min_mse_batch_dev: bad argument";
        return MSLAM_HIP_E_INVALID;
    }
    if(n_problems == 0)
        return MSLAM_HIP_OK;
    if(hipSetDevice(c->p.device) != hipSuccess)
    {
        c->err = "pnp_min_mse_batch_dev: hipSetDevice";
        return MSLAM_HIP_E_RUNTIME;
    }
    MseArgs a{};
    a.obj = d_object, a.img = d_image, a.n = d_n;
    a.n_problems = n_problems, a.capacity = capacity;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.pose = d_pose, a.info = d_info;
    {
        StageScope t(c, "pnp_min_mse");
        launch_min_mse(c, a, c->stream);
    }
    if(hipGetLastError() != hipSuccess)
    {
        c->err = "pnp_min_mse_batch_dev: launch failed";
        return MSLAM_HIP_E_RUNTIME;
    }
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_set_pnp_mse_loss(mslam_hip_ctx* c, int kind, double scale)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind < MSLAM_HIP_BA_LOSS_NONE || kind > MSLAM_HIP_BA_LOSS_CAUCHY)
        return mslam::fail(c, MSLAM_HIP_E_INVALID, "set_pnp_mse_loss: kind outside 0..2");
    if(kind != MSLAM_HIP_BA_LOSS_NONE && !(std::isfinite(scale) && scale > 0.0))
        return mslam::fail(c, MSLAM_HIP_E_INVALID, "set_pnp_mse_loss: the scale of HUBER / CAUCHY must be finite and > 0");
    c->mse_loss_kind = kind;
    c->mse_loss_scale = kind == MSLAM_HIP_BA_LOSS_NONE ? 0.0 : scale;
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_get_pnp_mse_loss(mslam_hip_ctx* c, int* kind, double* scale)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(kind)
        *kind = c->mse_loss_kind;
    if(scale)
        *scale = c->mse_loss_scale;
    return MSLAM_HIP_OK;
}
