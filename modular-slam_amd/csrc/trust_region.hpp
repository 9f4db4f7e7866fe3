// trust_region.hpp — what the Levenberg-Marquardt solves share: k_ba.hip (bundle adjustment), k_posegraph.hip (pose graph) and,
// for the constants and the reductions, k_pnp_mse.hip (a wave per problem, its loop in registers).
//
// The minimiser is Ceres 2.2's published trust-region loop (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc,
// trust_region_step_evaluator.cc, solver.cc) with the Solver::Options defaults of solver.h: monotonic steps, Jacobi scaling.
// In k_ba.hip and k_posegraph.hip one iteration is a fixed sequence of launches on the context's stream.  Every launch reads
// the control block (TrCtrl) first and returns when the solve has ended, so the host enqueues kTrBatch iterations ahead and
// looks at a mapped word between batches (tr_run).  Two one-wave kernels per solver carry the loop's decisions: the check
// kernel (FinalizeIterationAndCheckIfMinimizerCanContinue, tr_check) and the control kernel (step validity, the tolerances,
// accept or reject, the radius: tr_control).  Each scans its own parameter blocks and hands the lane-local results over.
// No sum uses an atomic and every sum has one order.  All arithmetic is f64, every expression rounds on its own
// (-ffp-contract=off), so a change of the order of operations here changes the bits of three solvers.
#pragma once
#include "context.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mslam
{

// Solver::Options defaults (solver.h); ceres::TerminationType
constexpr int kTrBatch = 4; // iterations enqueued between two looks at the termination word
constexpr int kTrMaxInvalidSteps = 5;
constexpr double kTrInitialRadius = 1e4, kTrMaxRadius = 1e16, kTrMinRadius = 1e-32;
constexpr double kTrMinDiagonal = 1e-6, kTrMaxDiagonal = 1e32;
constexpr double kTrMinRelativeDecrease = 1e-3;
constexpr double kTrFunctionTol = 1e-6, kTrGradientTol = 1e-10, kTrParameterTol = 1e-8;
constexpr int kTrConvergence = 0, kTrNoConvergence = 1, kTrFailure = 2;

struct TrCtrl
{
    int32_t done, termination, iteration, need_jac, first, successful, invalid_run, solve_bad;
    int32_t rejected, invalid_total, max_iterations, pad;
    double radius, decrease_factor, x_cost, initial_cost;
};

// ---- reductions ----------------------------------------------------------------------------------------------------------

// fixed-order butterfly: after the step with mask m, lanes l and l ^ m hold s_l + s_(l^m) = s_(l^m) + s_l, so every lane
// ends with the same bits
__device__ __forceinline__ double wave_sum(double s)
{
    for(int m = 32; m >= 1; m >>= 1)
        s += __shfl_xor(s, m, 64);
    return s;
}
__device__ __forceinline__ double wave_max(double s)
{
    for(int m = 32; m >= 1; m >>= 1)
        s = fmax(s, __shfl_xor(s, m, 64));
    return s;
}
// the sum of v over a block of 256, by a fixed tree: butterfly per wave, then the four waves in order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum(v);
    if((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
// entry (r, c) of a symmetric matrix kept as its upper triangle, row-major
__device__ __forceinline__ int tri6(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); } // r <= c < 6
__device__ __forceinline__ int tri3(int r, int c) { return r * 3 - r * (r - 1) / 2 + (c - r); } // r <= c < 3

// ---- the loss of the pose graph and of min-MSE PnP (k_ba.hip keeps its own ba_loss, the same formulas) -------------------

// what a loss form's launch carries: MSLAM_HIP_BA_LOSS_HUBER or _CAUCHY and its scale a
struct TrLoss
{
    int kind;
    double scale;
};
// loss_function.h's HuberLoss / CauchyLoss Evaluate at s = |r|^2 with scale a: rho(s) and w = rho'(s).  b = a^2.
//   HUBER:  s <= b: rho = s, w = 1 (s == b is the inlier branch); else rho = 2 a sqrt(s) - b, w = max(DBL_MIN, a / sqrt(s))
//   CAUCHY: rho = b log(1 + s / b), w = max(DBL_MIN, 1 / (1 + s / b)), s / b evaluated as s (1 / b)
// kind is MSLAM_HIP_BA_LOSS_HUBER or _CAUCHY (the callers keep NONE away).  rho'' <= 0 for both, so corrector.cc takes the
// branch that scales residual and Jacobians by sqrt(w) and nothing else.  s = 0 gives w = 1 in both (no 0 / 0); a NaN s
// gives a NaN rho, which the cost carries to FAILURE.
__device__ __forceinline__ void tr_loss(int kind, double a, double s, double& rho, double& w)
{
    const double b = a * a;
    if(kind == MSLAM_HIP_BA_LOSS_HUBER)
    {
        if(s <= b)
            rho = s, w = 1.0;
        else
        {
            const double r = sqrt(s);
            rho = 2.0 * a * r - b;
            w = fmax(DBL_MIN, a / r);
        }
    }
    else
    {
        const double sum = 1.0 + s * (1.0 / b);
        rho = b * log(sum);
        w = fmax(DBL_MIN, 1.0 / sum);
    }
}

// ---- quaternions, Eigen's x y z w ----------------------------------------------------------------------------------------

// Eigen's inverse(): conjugate / squared norm
__device__ __forceinline__ void quat_inverse(const double* __restrict__ q, double qi[4])
{
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    qi[0] = -q[0] / n2, qi[1] = -q[1] / n2, qi[2] = -q[2] / n2, qi[3] = q[3] / n2;
}
// Eigen's quaternion product
__device__ __forceinline__ void quat_product(const double a[4], const double b[4], double out[4])
{
    out[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    out[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    out[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    out[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
// Eigen's _transformVector: v + w uv + u x uv, uv = 2 (u x v)
__device__ __forceinline__ void quat_rotate(const double qi[4], const double v[3], double out[3])
{
    double uv[3] = {qi[1] * v[2] - qi[2] * v[1], qi[2] * v[0] - qi[0] * v[2], qi[0] * v[1] - qi[1] * v[0]};
    uv[0] += uv[0], uv[1] += uv[1], uv[2] += uv[2];
    out[0] = v[0] + qi[3] * uv[0] + (qi[1] * uv[2] - qi[2] * uv[1]);
    out[1] = v[1] + qi[3] * uv[1] + (qi[2] * uv[0] - qi[0] * uv[2]);
    out[2] = v[2] + qi[3] * uv[2] + (qi[0] * uv[1] - qi[1] * uv[0]);
}
// the matrix of v -> quat_rotate(qi, v): (1 - 2 |u|^2) I + 2 u u^T + 2 w [u]x, row-major
__device__ __forceinline__ void quat_matrix(const double qi[4], double Rt[9])
{
    const double x = qi[0], y = qi[1], z = qi[2], w = qi[3];
    const double xx = x * x, yy = y * y, zz = z * z;
    Rt[0] = 1.0 - 2.0 * (yy + zz), Rt[1] = 2.0 * (x * y - w * z), Rt[2] = 2.0 * (x * z + w * y);
    Rt[3] = 2.0 * (x * y + w * z), Rt[4] = 1.0 - 2.0 * (xx + zz), Rt[5] = 2.0 * (y * z - w * x);
    Rt[6] = 2.0 * (x * z - w * y), Rt[7] = 2.0 * (y * z + w * x), Rt[8] = 1.0 - 2.0 * (xx + yy);
}
// EigenQuaternionManifold::Plus (manifold.h QuaternionPlus): q_delta (x) q
__device__ __forceinline__ void quat_plus(const double* __restrict__ q, const double d[3], double out[4])
{
    const double norm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if(!(norm > 0.0))
    {
        out[0] = q[0], out[1] = q[1], out[2] = q[2], out[3] = q[3];
        return;
    }
    const double sbd = sin(norm) / norm;
    const double ax = sbd * d[0], ay = sbd * d[1], az = sbd * d[2], aw = cos(norm);
    out[0] = aw * q[0] + ax * q[3] + ay * q[2] - az * q[1];
    out[1] = aw * q[1] + ay * q[3] + az * q[0] - ax * q[2];
    out[2] = aw * q[2] + az * q[3] + ax * q[1] - ay * q[0];
    out[3] = aw * q[3] - ax * q[0] - ay * q[1] - az * q[2];
}

// ---- one pose block (q, p), tangent (delta, dp) ----------------------------------------------------------------------------

// the check kernels' scan of a pose x with the gradient g (6) and the 21 entries U of J^T J: |x - Plus(x, -g)|_inf over the
// seven ambient parameters into gmax, and whether the evaluation is usable into ok.  ResidualBlock::Evaluate rejects
// non-finite residuals or Jacobian entries; any such entry makes the cost, a gradient entry or a diagonal entry of J^T J (a
// sum of squares) non-finite (DEVIATES `evaluation valid` in include/mslam_hip.h)
__device__ __forceinline__ void tr_pose_gradient(const double* __restrict__ x, const double* __restrict__ g, const double* __restrict__ U,
                                                 bool& ok, double& gmax)
{
    const double md[3] = {-g[0], -g[1], -g[2]};
    double qp[4];
    quat_plus(x, md, qp);
    for(int j = 0; j < 4; ++j)
        gmax = fmax(gmax, fabs(x[j] - qp[j]));
    for(int j = 0; j < 3; ++j)
        gmax = fmax(gmax, fabs(x[4 + j] - (x[4 + j] + (-g[3 + j]))));
    for(int j = 0; j < 6; ++j)
        ok = ok && isfinite(g[j]) && isfinite(U[tri6(j, j)]);
}
// the candidate c = Plus(x, delta) with delta = step * scaling, step = -y; y = nullptr: a pose outside the problem, copied
__device__ __forceinline__ void tr_pose_plus(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ sc,
                                             double* __restrict__ c)
{
    if(!y)
    {
        for(int j = 0; j < 7; ++j)
            c[j] = x[j];
        return;
    }
    const double d[3] = {-y[0] * sc[0], -y[1] * sc[1], -y[2] * sc[2]};
    double q[4];
    quat_plus(x, d, q);
    c[0] = q[0], c[1] = q[1], c[2] = q[2], c[3] = q[3];
    for(int j = 0; j < 3; ++j)
        c[4 + j] = x[4 + j] + (-y[3 + j] * sc[3 + j]);
}
// the control kernels' scan of a pose x, its candidate and its solution y (6): the step is finite; |x|^2 and
// |x - candidate|^2 over the seven ambient parameters
__device__ __forceinline__ void tr_pose_step(const double* __restrict__ x, const double* __restrict__ cand, const double* __restrict__ y,
                                             bool& finite, double& xn, double& sn)
{
    for(int j = 0; j < 6; ++j)
        finite = finite && isfinite(y[j]);
    for(int j = 0; j < 7; ++j)
    {
        const double v = x[j], d = v - cand[j];
        xn += v * v, sn += d * d;
    }
}

// ---- the loop's decisions: one wave each ---------------------------------------------------------------------------------

__device__ __forceinline__ void tr_finish(TrCtrl* ct, int32_t* h_done, int lane, int termination)
{
    if(lane == 0)
    {
        ct->termination = termination;
        ct->done = 1;
        *h_done = 1; // mapped: the host's look between batches
    }
}

// FinalizeIterationAndCheckIfMinimizerCanContinue, after the caller's scan of its parameter blocks: ok and gmax are the
// lane's own; part is [2][n_blocks] from the eval kernel, whose second row is the cost at the start in iteration 0
__device__ __forceinline__ void tr_check(TrCtrl* ct, int32_t* h_done, int lane, const double* __restrict__ part, int n_blocks, bool ok,
                                         double gmax)
{
    double x_cost = ct->x_cost;
    if(ct->first)
    {
        double s = 0.0;
        for(int b = lane; b < n_blocks; b += 64)
            s += part[n_blocks + b];
        x_cost = wave_sum(s);
    }
    gmax = wave_max(gmax);
    ok = __all(ok && isfinite(x_cost));
    if(lane == 0 && ct->first)
        ct->x_cost = ct->initial_cost = x_cost;
    if(!ok)
        return tr_finish(ct, h_done, lane, kTrFailure);
    if(ct->iteration >= ct->max_iterations)
        return tr_finish(ct, h_done, lane, kTrNoConvergence);
    if(ct->successful && gmax <= kTrGradientTol)
        return tr_finish(ct, h_done, lane, kTrConvergence);
    if(ct->radius <= kTrMinRadius)
        return tr_finish(ct, h_done, lane, kTrConvergence);
    if(lane == 0)
    {
        ct->iteration += 1;
        ct->successful = 0;
        ct->first = 0;
        ct->solve_bad = 0;
    }
}

// The bookkeeping of one iteration, after the caller's scan of its parameter blocks: finite, xn = |x|^2 and sn =
// |x - candidate|^2 are the lane's own; part is [2][n_blocks]: model cost change, candidate cost.  Sums in a fixed order, step
// validity, parameter / function tolerance, accept or reject, radius.  True, in every lane, when the step is accepted: the
// caller then copies its candidate into its state
__device__ __forceinline__ bool tr_control(TrCtrl* ct, int32_t* h_done, int lane, const double* __restrict__ part, int n_blocks,
                                           bool finite, double xn, double sn)
{
    double ms = 0.0, cs = 0.0;
    for(int b = lane; b < n_blocks; b += 64)
        ms += part[b], cs += part[n_blocks + b];
    const double model_cost_change = wave_sum(ms);
    double cand_cost = wave_sum(cs);
    finite = __all(finite);
    const double x_norm = sqrt(wave_sum(xn)), step_norm = sqrt(wave_sum(sn));
    const double x_cost = ct->x_cost;
    double radius = ct->radius, decrease_factor = ct->decrease_factor;
    if(!(finite && !ct->solve_bad && model_cost_change > 0.0))
    {
        // HandleInvalidStep
        if(lane == 0)
            ct->invalid_total += 1;
        if(ct->invalid_run + 1 >= kTrMaxInvalidSteps)
        {
            tr_finish(ct, h_done, lane, kTrFailure);
            return false;
        }
        if(lane == 0)
        {
            ct->invalid_run += 1;
            ct->radius = radius / decrease_factor; // StepIsInvalid = StepRejected(0)
            ct->decrease_factor = decrease_factor * 2.0;
            ct->need_jac = 0;
        }
        return false;
    }
    // a candidate that fails to evaluate is a step of infinite cost (ComputeCandidatePointAndEvaluateCost)
    if(!isfinite(cand_cost))
        cand_cost = DBL_MAX;
    if(lane == 0)
        ct->invalid_run = 0;
    if(step_norm <= kTrParameterTol * (x_norm + kTrParameterTol) || fabs(x_cost - cand_cost) <= kTrFunctionTol * x_cost)
    {
        tr_finish(ct, h_done, lane, kTrConvergence);
        return false;
    }
    // IsStepSuccessful (monotonic: the step evaluator's reference cost is the current cost)
    const double relative_decrease = cand_cost >= DBL_MAX ? -DBL_MAX : (x_cost - cand_cost) / model_cost_change;
    const bool accepted = relative_decrease > kTrMinRelativeDecrease;
    if(lane != 0)
        return accepted;
    if(accepted)
    {
        const double q = 2.0 * relative_decrease - 1.0;
        radius = radius / fmax(1.0 / 3.0, 1.0 - q * q * q);
        ct->radius = fmin(kTrMaxRadius, radius);
        ct->decrease_factor = 2.0;
        ct->x_cost = cand_cost;
        ct->successful = 1;
        ct->need_jac = 1;
    }
    else
    {
        ct->rejected += 1;
        ct->radius = radius / decrease_factor;
        ct->decrease_factor = decrease_factor * 2.0;
        ct->need_jac = 0;
    }
    return accepted;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

// the entry points' test of a quaternion of the caller's
inline bool tr_unit_quaternion(const double* q)
{
    const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    return std::fabs(norm - 1.0) <= 1e-6;
}

// One device block of a solve, carved in 16-byte steps: first what is uploaded (put: the control block at 0, the problem),
// then the working arrays (carve).  The offsets hold for the device block, which the caller grows to `size` bytes.  put keeps
// the caller's pointer until upload, which copies everything into one host block (padding zeroed) and enqueues one transfer.
struct TrStaging
{
    struct Span
    {
        size_t at;
        const void* src;
        size_t bytes;
    };
    size_t size = 0, head = 0; // bytes carved; bytes of the uploaded head
    TrCtrl ctrl{};
    std::vector<Span> spans;
    std::vector<uint8_t> host;

    explicit TrStaging(int max_iterations)
    {
        ctrl.need_jac = 1, ctrl.first = 1, ctrl.successful = 1, ctrl.max_iterations = max_iterations;
        ctrl.radius = kTrInitialRadius, ctrl.decrease_factor = 2.0;
        put(&ctrl, sizeof(ctrl));
    }
    TrStaging(const TrStaging&) = delete; // a span points at ctrl
    size_t carve(size_t bytes)
    {
        const size_t at = size;
        size += (bytes + 15) & ~(size_t)15;
        return at;
    }
    size_t put(const void* src, size_t bytes) // before the first carve of a working array
    {
        spans.push_back({carve(bytes), src, bytes});
        head = size;
        return spans.back().at;
    }
    hipError_t upload(uint8_t* d, hipStream_t s)
    {
        host.assign(head, 0);
        for(const Span& p : spans)
            if(p.bytes)
                std::memcpy(&host[p.at], p.src, p.bytes);
        return hipMemcpyAsync(d, host.data(), head, hipMemcpyHostToDevice, s);
    }
};

// The batch loop of a solve whose start cost is enqueued: kTrBatch calls of enqueue_iteration, then a look at the mapped word
// the kernels set with the termination (the context's h_ba); at the end the control block comes back and fills `sum`.
// `stage` names the timed stage of a batch, `who` the entry point in the error.  MSLAM_HIP_OK also for a solve that ended in
// FAILURE (sum.termination).
template <class Enqueue>
int tr_run(mslam_hip_ctx* c, const char* stage, const char* who, const TrCtrl* d_ctrl, int max_iterations, Enqueue&& enqueue_iteration,
           mslam_hip_ba_summary& sum)
{
    hipStream_t s = c->stream;
    // iteration max_iterations + 1 only reaches the check kernel, which ends the solve with NO_CONVERGENCE
    for(long long it = 0; it <= max_iterations;) // a wide counter: max_iterations + 1 must not wrap for INT_MAX
    {
        StageScope ts(c, stage);
        for(int b = 0; b < kTrBatch && it <= max_iterations; ++b, ++it)
            enqueue_iteration();
        MSLAM_CHK(c, hipGetLastError());
        MSLAM_CHK(c, hipStreamSynchronize(s));
        if(*static_cast<volatile int32_t*>(c->h_ba.get()))
            break;
    }
    TrCtrl ctrl;
    MSLAM_CHK(c, hipMemcpyAsync(&ctrl, d_ctrl, sizeof(ctrl), hipMemcpyDeviceToHost, s));
    MSLAM_CHK(c, hipStreamSynchronize(s));
    if(!ctrl.done)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": the kernels left no termination");
    sum.termination = ctrl.termination, sum.iterations = ctrl.iteration;
    sum.rejected_steps = ctrl.rejected, sum.invalid_steps = ctrl.invalid_total;
    sum.initial_cost = ctrl.initial_cost, sum.final_cost = ctrl.x_cost;
    return MSLAM_HIP_OK;
}

} // namespace mslam
