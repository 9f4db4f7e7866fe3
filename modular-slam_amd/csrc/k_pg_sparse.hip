// k_pg_sparse.hip — the pose graph's sparse linear solver: a Cholesky factor of the damped normal equations on their block
// envelope (skyline) in 6 x 6 blocks, after a deterministic ordering.  Memory and work follow the envelope, not K^2.
// DESIGN.md 4.25 has the walk-through; include/mslam_hip.h the ordering rule.
//
// Symbolic phase (host, per call): pg_symbolic computes the NATURAL and the RCM order of the free poses that have an edge and
// keeps the one with the smaller envelope; pg_layout gives every row its offset and every column the list of the rows whose
// envelope holds it.  mslam_hip_pose_graph_analyze exposes the first without a context.  mslam_hip_bundle_adjust_global's
// SPARSE solver (k_ba.hip) uses both, with a node mask, and the three kernels below on its reduced camera system.
//
// Numeric phase: row i of the lower triangle lies contiguously from column first[i] to i; the right-hand side is one more
// block column, kept in rhs.  Four launches per solve on one stream; each reads the control block first:
//   k_pgs_clear      zeroes the envelope
//   (the caller's assembly: k_pg_assemble_env of k_posegraph.hip)
//   k_pgs_factor     ONE workgroup of 256 walks the block columns in order.  The chain of dependencies of an envelope factor
//                    is as long as the matrix has block rows (a chain of poses has no level parallelism), so a launch per
//                    level would be a launch per pose.  For column j:
//                      1. every wave factors the diagonal block in registers (lane r < 6 owns row r, lane 6 the right-hand
//                         side's row, values pass by shuffles; the four waves compute the same bits), so no barrier is
//                         needed before every thread holds L_jj and y_j;
//                      2. L_ij = A_ij L_jj^-T for the rows i of the column's list: a thread per row of a block;  barrier (only
//                         after it does wave 0 write L_jj and y_j over what the other waves have read);
//                      3. A_ik -= L_ij L_kj^T over the pairs i >= k > j of those rows and b_i -= L_ij y_j: a thread per
//                         entry;  barrier.
//                    Every entry receives its updates in ascending j, one per column, each from exactly one thread: no
//                    atomics, one order of every sum.
//   k_pgs_backsolve  ONE workgroup sweeps the rows from the last to the first: every thread solves L_ii^T x_i = y_i (the same
//                    bits), then y_k -= L_ik^T x_i for the row's columns k, a thread per entry;  barrier.
// No kernel waits on another workgroup; every loop is bounded by a count the host computed (n, the lists' lengths, the
// rows' widths).  All arithmetic is f64.  The diagonal's reciprocal is taken once per column and multiplied with.
// mslam_hip_pose_graph_covariance stops after the factor (pg_sparse_factor) and goes on in k_pg_cov.hip.
#include "pg_sparse.hpp"

#include <algorithm>

namespace mslam
{

__global__ __launch_bounds__(256) void k_pgs_clear(PgsArgs a)
{
    if(a.ctrl->done)
        return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if(i < (size_t)a.blocks * 36)
        a.S[i] = 0.0;
}

__device__ __forceinline__ int pgs_tri(int c, int k) { return c * (c + 1) / 2 + k; } // k <= c < 6

__global__ __launch_bounds__(256) void k_pgs_factor(PgsArgs a)
{
    TrCtrl* ct = a.ctrl;
    if(ct->done)
        return;
    const int t = threadIdx.x, lane = t & 63;
    bool bad = false;
    for(int j = 0; j < a.n; ++j)
    {
        // 1. the diagonal block: lane r < 6 of every wave holds row r of the lower triangle, lane 6 the right-hand side
        double* D = a.S + (size_t)(a.row_off[j] + j - a.first[j]) * 36;
        double v[6], inv[6];
#pragma unroll
        for(int c = 0; c < 6; ++c)
        {
            v[c] = 0.0;
            if(lane < 6 && c <= lane)
                v[c] = D[lane * 6 + c];
            else if(lane == 6)
                v[c] = a.rhs[(size_t)j * 6 + c];
        }
#pragma unroll
        for(int jj = 0; jj < 6; ++jj)
        {
            double x = v[jj];
#pragma unroll
            for(int k = 0; k < jj; ++k)
                x -= v[k] * __shfl(v[k], jj, 64);
            const double d = __shfl(x, jj, 64);
            if(!(d > 0.0) || !isfinite(d))
                bad = true; // the step is invalid; the factorisation goes on with bounded values
            const double sd = sqrt(fmax(d, DBL_MIN));
            inv[jj] = 1.0 / sd;
            v[jj] = lane == jj ? sd : x * inv[jj];
        }
        double L[21], y[6];
#pragma unroll
        for(int c = 0; c < 6; ++c)
        {
#pragma unroll
            for(int k = 0; k <= c; ++k)
                L[pgs_tri(c, k)] = __shfl(v[k], c, 64);
            y[c] = __shfl(v[c], 6, 64);
        }
        // 2. the rows below
        const int cp = a.col_ptr[j], m = a.col_ptr[j + 1] - cp;
        for(int w = t; w < 6 * m; w += 256)
        {
            double* P = a.S + (size_t)a.col_blk[cp + w / 6] * 36 + (w % 6) * 6;
            double x[6];
#pragma unroll
            for(int c = 0; c < 6; ++c)
                x[c] = P[c];
#pragma unroll
            for(int c = 0; c < 6; ++c)
            {
                double s = x[c];
#pragma unroll
                for(int k = 0; k < c; ++k)
                    s -= x[k] * L[pgs_tri(c, k)];
                x[c] = s * inv[c];
            }
#pragma unroll
            for(int c = 0; c < 6; ++c)
                P[c] = x[c];
        }
        __syncthreads();
        // every wave has read the diagonal block and the right-hand side by now: wave 0 writes L_jj and y_j over them (the
        // update below touches neither)
        if(t < 6)
        {
#pragma unroll
            for(int c = 0; c < 6; ++c)
                if(c <= t)
                    D[t * 6 + c] = v[c];
        }
        else if(t == 6)
        {
#pragma unroll
            for(int c = 0; c < 6; ++c)
            {
                a.rhs[(size_t)j * 6 + c] = v[c];
                a.dinv[(size_t)j * 6 + c] = inv[c];
            }
        }
        // 3. the trailing update: m (m + 1) / 2 blocks of 36 entries (the host bounds that by the envelope), then 6 m entries of
        // the right-hand side
        const int n_pair = m * (m + 1) / 2, n_item = n_pair * 36 + 6 * m;
        for(int w = t; w < n_item; w += 256)
        {
            if(w >= n_pair * 36)
            {
                const int u = w - n_pair * 36, p = u / 6, r = u % 6;
                const double* Lp = a.S + (size_t)a.col_blk[cp + p] * 36 + r * 6;
                double s = 0.0;
#pragma unroll
                for(int k = 0; k < 6; ++k)
                    s += Lp[k] * y[k];
                a.rhs[(size_t)a.col_row[cp + p] * 6 + r] -= s;
                continue;
            }
            const int b = w / 36, e = w % 36, r = e / 6, c = e % 6;
            int p = (int)((sqrt(8.0 * b + 1.0) - 1.0) / 2.0);
            if(p * (p + 1) / 2 > b) // the root rounded up or down by one: at most one step either way
                --p;
            else if((p + 1) * (p + 2) / 2 <= b)
                ++p;
            const int q = b - p * (p + 1) / 2;
            if(p < 0 || p >= m || q < 0 || q > p)
                continue; // cannot happen for w < n_item: no entry outside the envelope is ever written
            const int bp = a.col_blk[cp + p];
            const double* Lp = a.S + (size_t)bp * 36 + r * 6;
            const double* Lq = a.S + (size_t)a.col_blk[cp + q] * 36 + c * 6;
            double s = 0.0;
#pragma unroll
            for(int k = 0; k < 6; ++k)
                s += Lp[k] * Lq[k];
            a.S[(size_t)(bp + (a.col_row[cp + q] - j)) * 36 + r * 6 + c] -= s;
        }
        __syncthreads();
    }
    if(bad && t == 0)
        ct->solve_bad = 1;
}

__global__ __launch_bounds__(256) void k_pgs_backsolve(PgsArgs a)
{
    if(a.ctrl->done)
        return;
    const int t = threadIdx.x;
    for(int i = a.n - 1; i >= 0; --i)
    {
        const int f = a.first[i];
        const double* Rw = a.S + (size_t)a.row_off[i] * 36;
        const double* D = Rw + (size_t)(i - f) * 36;
        double x[6];
#pragma unroll
        for(int c = 0; c < 6; ++c)
            x[c] = a.rhs[(size_t)i * 6 + c];
#pragma unroll
        for(int c = 5; c >= 0; --c)
        {
            double s = x[c];
#pragma unroll
            for(int k = c + 1; k < 6; ++k)
                s -= D[k * 6 + c] * x[k];
            x[c] = s * a.dinv[(size_t)i * 6 + c];
        }
        if(t == 0)
        {
#pragma unroll
            for(int c = 0; c < 6; ++c)
                a.yc[(size_t)i * 6 + c] = x[c];
        }
        for(int w = t; w < (i - f) * 6; w += 256)
        {
            const int cb = w / 6, r = w % 6;
            const double* B = Rw + (size_t)cb * 36;
            double s = 0.0;
#pragma unroll
            for(int k = 0; k < 6; ++k)
                s += B[k * 6 + r] * x[k];
            a.rhs[(size_t)(f + cb) * 6 + r] -= s;
        }
        __syncthreads();
    }
}

void pg_sparse_factor(mslam_hip_ctx* c, const PgsArgs& a, hipStream_t s, const std::function<void()>& assemble)
{
    {
        StageScope tk(c, "solver_schur");
        hipLaunchKernelGGL(k_pgs_clear, dim3((unsigned)(((size_t)a.blocks * 36 + 255) / 256)), dim3(256), 0, s, a);
        assemble();
    }
    StageScope tk(c, "solver_factor");
    hipLaunchKernelGGL(k_pgs_factor, dim3(1), dim3(256), 0, s, a);
}

void pg_sparse_solve(mslam_hip_ctx* c, const PgsArgs& a, hipStream_t s, const std::function<void()>& assemble)
{
    pg_sparse_factor(c, a, s, assemble);
    StageScope tk(c, "solver_subst");
    hipLaunchKernelGGL(k_pgs_backsolve, dim3(1), dim3(256), 0, s, a);
}

// ---- the symbolic phase ------------------------------------------------------------------------------------------------------

// first[] and the envelope of an order; pos: [K] position per pose
static int64_t pg_envelope(const std::vector<int32_t>& order, const std::vector<int32_t>& adj_ptr, const std::vector<int32_t>& adj,
                           std::vector<int32_t>& pos, std::vector<int32_t>& first)
{
    const int n = (int)order.size();
    for(int i = 0; i < n; ++i)
        pos[(size_t)order[(size_t)i]] = i;
    first.assign((size_t)n, 0);
    int64_t blocks = 0;
    for(int i = 0; i < n; ++i)
    {
        const int k = order[(size_t)i];
        int f = i;
        for(int at = adj_ptr[(size_t)k]; at < adj_ptr[(size_t)k + 1]; ++at)
            f = std::min(f, pos[(size_t)adj[(size_t)at]]);
        first[(size_t)i] = f;
        blocks += i - f + 1;
    }
    return blocks;
}

void pg_symbolic(const uint8_t* fixed, int K, const int32_t* edge_a, const int32_t* edge_b, size_t E, PgSymbolic& sy,
                 const uint8_t* node_mask)
{
    std::vector<uint8_t> node((size_t)K, 0);
    if(node_mask)
        node.assign(node_mask, node_mask + K);
    else
        for(size_t e = 0; e < E; ++e)
            node[(size_t)edge_a[e]] = node[(size_t)edge_b[e]] = 1;
    std::vector<int32_t> natural;
    for(int k = 0; k < K; ++k)
    {
        node[(size_t)k] = node[(size_t)k] && !(fixed && fixed[k]);
        if(node[(size_t)k])
            natural.push_back(k);
    }
    const int n = (int)natural.size();
    // the neighbours of every node, ascending, duplicates once, constant poses left out
    std::vector<std::pair<int32_t, int32_t>> pr;
    for(size_t e = 0; e < E; ++e)
        if(node[(size_t)edge_a[e]] && node[(size_t)edge_b[e]])
            pr.push_back({edge_a[e], edge_b[e]}), pr.push_back({edge_b[e], edge_a[e]});
    std::sort(pr.begin(), pr.end());
    pr.erase(std::unique(pr.begin(), pr.end()), pr.end());
    std::vector<int32_t> adj_ptr((size_t)K + 1, 0), adj(pr.size());
    for(size_t i = 0; i < pr.size(); ++i)
        ++adj_ptr[(size_t)pr[i].first + 1], adj[i] = pr[i].second;
    for(int k = 0; k < K; ++k)
        adj_ptr[(size_t)k + 1] += adj_ptr[(size_t)k];
    auto degree = [&](int k) { return adj_ptr[(size_t)k + 1] - adj_ptr[(size_t)k]; };
    auto by_degree = [&](int x, int y) { return degree(x) != degree(y) ? degree(x) < degree(y) : x < y; };
    // reverse Cuthill-McKee: components one after another, each from its unvisited node of least degree (ties: the smallest
    // index), breadth first, the unvisited neighbours of the node being expanded in ascending (degree, index); all reversed
    std::vector<int32_t> starts(natural), rcm, next;
    std::sort(starts.begin(), starts.end(), by_degree);
    std::vector<uint8_t> seen((size_t)K, 0);
    rcm.reserve((size_t)n);
    size_t head = 0;
    for(const int32_t s0 : starts)
    {
        if(seen[(size_t)s0])
            continue;
        seen[(size_t)s0] = 1;
        rcm.push_back(s0);
        while(head < rcm.size())
        {
            const int u = rcm[head++];
            next.clear();
            for(int at = adj_ptr[(size_t)u]; at < adj_ptr[(size_t)u + 1]; ++at)
                if(!seen[(size_t)adj[(size_t)at]])
                    seen[(size_t)adj[(size_t)at]] = 1, next.push_back(adj[(size_t)at]);
            std::sort(next.begin(), next.end(), by_degree);
            rcm.insert(rcm.end(), next.begin(), next.end());
        }
    }
    std::reverse(rcm.begin(), rcm.end());
    std::vector<int32_t> pos((size_t)K, -1), first_nat, first_rcm;
    const int64_t b_nat = pg_envelope(natural, adj_ptr, adj, pos, first_nat);
    const int64_t b_rcm = pg_envelope(rcm, adj_ptr, adj, pos, first_rcm);
    sy.n_free = n;
    sy.ordering = b_rcm < b_nat ? 1 : 0; // NATURAL on a tie
    sy.blocks = sy.ordering ? b_rcm : b_nat;
    sy.order = sy.ordering ? std::move(rcm) : std::move(natural);
    sy.first = sy.ordering ? std::move(first_rcm) : std::move(first_nat);
}

void pg_layout(PgSymbolic& sy)
{
    const int n = sy.n_free;
    sy.row_off.assign((size_t)n, 0);
    sy.col_ptr.assign((size_t)n + 1, 0);
    int32_t at = 0;
    for(int i = 0; i < n; ++i)
    {
        sy.row_off[(size_t)i] = at;
        at += i - sy.first[(size_t)i] + 1;
        for(int j = sy.first[(size_t)i]; j < i; ++j)
            ++sy.col_ptr[(size_t)j + 1];
    }
    for(int j = 0; j < n; ++j)
        sy.col_ptr[(size_t)j + 1] += sy.col_ptr[(size_t)j];
    sy.col_blk.assign((size_t)sy.col_ptr[(size_t)n], 0);
    sy.col_row.assign((size_t)sy.col_ptr[(size_t)n], 0);
    std::vector<int32_t> fill(sy.col_ptr.begin(), sy.col_ptr.end() - 1);
    for(int i = 0; i < n; ++i) // rows ascending: every column's list is ascending
        for(int j = sy.first[(size_t)i]; j < i; ++j)
        {
            const int32_t slot = fill[(size_t)j]++;
            sy.col_blk[(size_t)slot] = sy.row_off[(size_t)i] + j - sy.first[(size_t)i];
            sy.col_row[(size_t)slot] = i;
        }
}

int pg_symbolic_out(const PgSymbolic& sy, int32_t* order, int32_t* first, int* n_free, int* ordering, int64_t* envelope_blocks)
{
    for(int i = 0; i < sy.n_free; ++i)
    {
        if(order)
            order[i] = sy.order[(size_t)i];
        if(first)
            first[i] = sy.first[(size_t)i];
    }
    if(n_free)
        *n_free = sy.n_free;
    if(ordering)
        *ordering = sy.ordering;
    if(envelope_blocks)
        *envelope_blocks = sy.blocks;
    return sy.blocks > MSLAM_HIP_POSE_GRAPH_MAX_ENVELOPE_BLOCKS ? MSLAM_HIP_E_CAPACITY : MSLAM_HIP_OK;
}

} // namespace mslam

using namespace mslam;

extern "C" int mslam_hip_pose_graph_analyze(const uint8_t* fixed, int K, const int32_t* edge_a, const int32_t* edge_b, int E,
                                            int32_t* order, int32_t* first, int* n_free, int* ordering, int64_t* envelope_blocks)
{
    if(K < 0 || K > MSLAM_HIP_POSE_GRAPH_MAX_KEYFRAMES_SPARSE || E < 0 || E > MSLAM_HIP_POSE_GRAPH_MAX_EDGES)
        return MSLAM_HIP_E_INVALID;
    if(E > 0 && (!edge_a || !edge_b))
        return MSLAM_HIP_E_INVALID;
    for(int e = 0; e < E; ++e)
        if(edge_a[e] < 0 || edge_a[e] >= K || edge_b[e] < 0 || edge_b[e] >= K || edge_a[e] == edge_b[e])
            return MSLAM_HIP_E_INVALID;
    PgSymbolic sy;
    pg_symbolic(fixed, K, edge_a, edge_b, E, sy);
    return pg_symbolic_out(sy, order, first, n_free, ordering, envelope_blocks);
}
