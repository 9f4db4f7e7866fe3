// k_match_guided.hip — guided matching: every landmark is matched among the keypoints inside a square window round its
// projection under a pose guess, instead of among all keypoints of the frame (the semantics are stated once, at
// mslam_hip_match_guided_knn2 in include/mslam_hip.h).
//
// The reference matches brute force (matchLandmarks, rgbd_feature_frontend.cpp:237-254, with the note
// "TODO: use boost geometry rtree for keypoints" at :242) although track() projects every matched landmark with the current
// pose (:300); this is the matcher that projection makes possible.
//
//   k_guided_bin     one workgroup per row: counting sort of the row's in-frame keypoints into square cells (LDS
//                    histogram, scan, scatter) -> cell offsets + a list per row that holds, cell by cell, each keypoint's
//                    coordinates, index and a copy of its descriptor (the matcher's gather is latency-bound: with the
//                    copies a list position is all it needs, one level of dependent fetches instead of three)
//   k_match_guided   eight lanes per landmark: project once, visit the cell rows the window overlaps (the cells of one cell
//                    row are one contiguous span of the list), each lane tests one listed keypoint at a time — exact window
//                    membership, then xor / popcount over its 32 bytes — and keeps two minima of dist << 16 | index; the
//                    eight lanes' minima are merged by a butterfly.  The key makes the result independent of the cell
//                    size and of the order inside a cell (the scatter's order is not deterministic).
//   k_ratio_guided   the acceptance test and the ordered compaction (k_ratio_compact's, with the distance gate, a lone
//                    candidate accepted, and no "fewer than two train rows" rule)
//
// The projection, the binning body and the walk are guided_walk.hpp's, which landmark fusion (k_fuse.hip, k_fuse_multi.hip)
// uses as well.  All projection arithmetic is f64, every operation rounded on its own (-ffp-contract=off), in the order written.
#include "guided_walk.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

namespace mslam
{

namespace
{
__device__ __forceinline__ int guided_row_kp(const GuidedArgs& a, int row)
{
    return min(max(a.kp_cnt ? a.kp_cnt[row] : a.n_kp_fixed, 0), a.kp_cap);
}
} // namespace

// one workgroup per row
__global__ __launch_bounds__(kGuidedBinThreads) void k_guided_bin(GuidedArgs a)
{
    const size_t row = blockIdx.x;
    guided_bin_row(GuidedBinRow{a.kp_xy + row * a.kp_stride * 2, a.kp_desc + row * a.kp_stride * 32, guided_row_kp(a, (int)row),
                                a.cell_off + row * (kGuidedMaxCells + 1), a.list + row * a.kp_cap, a.list_desc + row * a.kp_cap * 32},
                   a.width, a.height, a.grid);
}

// 64 or 256 threads: 8 or 32 landmarks per workgroup
__global__ __launch_bounds__(256) void k_match_guided(GuidedArgs a)
{
    const int row = blockIdx.y, g = threadIdx.x & 7;
    const int j = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
    const int n_lm = min(max(a.lm_cnt ? a.lm_cnt[row] : a.n_lm_fixed, 0), a.cap);
    const bool live = j < n_lm; // (the eight lanes of a landmark agree)
    GuidedUV p{0.0, 0.0, 0.0};
    if(live)
        p = guided_project(a.R, a.t, a.fx, a.fy, a.cx, a.cy,
                           a.world + (a.slots ? (size_t)a.slots[(size_t)row * a.slot_stride] * a.world_slot : 0) + (size_t)j * 3);
    uint32_t cnt = 0; // every keypoint inside the window is a candidate
    const uint2 k = guided_walk<true>(live && p.c2 > 0.0, p.u, p.v, a.radius, a.width, a.height, a.grid, a.cell_off + (size_t)row * (kGuidedMaxCells + 1),
                                a.list + (size_t)row * a.kp_cap, a.list_desc + (size_t)row * a.kp_cap * 32,
                                a.lm_desc + (size_t)row * a.lm_stride + (size_t)j * 32, g, [&cnt](int) {
                                    ++cnt;
                                    return true;
                                });
    for(int o = 1; o < 8; o <<= 1)
        cnt += __shfl_xor(cnt, o);
    if(live && g == 0)
    {
        const uint32_t k0 = k.x, k1 = k.y;
        const size_t o = (size_t)row * a.cap + j;
        a.idx0[o] = k0 == ~0u ? -1 : (int32_t)(k0 & 0xFFFFu);
        a.idx1[o] = k1 == ~0u ? -1 : (int32_t)(k1 & 0xFFFFu);
        a.dist0[o] = k0 == ~0u ? INT_MAX : (int32_t)(k0 >> 16);
        a.dist1[o] = k1 == ~0u ? INT_MAX : (int32_t)(k1 >> 16);
        if(a.n_cand)
            a.n_cand[o] = (int32_t)cnt;
    }
}

// one workgroup per row: d0 <= max_distance && (no second candidate || d0 < thr[d1]), ordered compaction.  An absent
// distance is INT_MAX: an absent d0 fails the gate (max_distance <= 256), an absent d1 never indexes the table.
__global__ __launch_bounds__(256) void k_ratio_guided(RatioArgs a, int max_distance)
{
    __shared__ uint32_t wcnt[4];
    const int pair = blockIdx.x;
    const int n_to = min(max(a.to_cnt ? a.to_cnt[pair] : a.n_to_fixed, 0), a.cap);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t o = (size_t)pair * a.cap;
    uint32_t base = 0;
    for(int q0 = 0; q0 < n_to; q0 += 256)
    {
        const int q = q0 + tid;
        bool ok = false;
        int fi = -1;
        if(q < n_to)
        {
            const int d0 = a.dist0[o + q], d1 = a.dist1[o + q];
            fi = a.idx0[o + q];
            ok = d0 <= max_distance && ((unsigned)d1 > 256u || d0 < a.thr[d1]);
        }
        const unsigned long long b = __ballot(ok);
        if(lane == 0)
            wcnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int w = 0; w < 4; ++w)
        {
            if(w < wave)
                pre += wcnt[w];
            tot += wcnt[w];
        }
        if(ok)
        {
            const uint32_t pos = base + pre + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
            a.from_idx[o + pos] = fi;
            a.to_idx[o + pos] = q;
        }
        base += tot;
        __syncthreads();
    }
    if(tid == 0)
        a.n_out[pair] = (int32_t)base;
}

void launch_guided_bin(const GuidedArgs& a, int rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_guided_bin, dim3((unsigned)rows), dim3(kGuidedBinThreads), 0, s, a);
}

void launch_match_guided(const GuidedArgs& a, int rows, hipStream_t s)
{
    // one wave per workgroup spreads a single row over the chip; many rows take four waves per workgroup (a quarter of
    // the workgroups to dispatch)
    const int block = (long long)rows * ((a.cap + 7) / 8) > 4096 ? 256 : 64, per = block / 8;
    hipLaunchKernelGGL(k_match_guided, dim3((unsigned)((a.cap + per - 1) / per), (unsigned)rows), dim3(block), 0, s, a);
}

void launch_ratio_guided(const RatioArgs& a, int max_distance, int n_pairs, hipStream_t s)
{
    hipLaunchKernelGGL(k_ratio_guided, dim3((unsigned)n_pairs), dim3(256), 0, s, a, max_distance);
}

} // namespace mslam

using namespace mslam;

// ---- host side ---------------------------------------------------------------------------------------------------------

namespace
{
bool bad_extent(int v) { return v < 1 || v > 8192; }

// the arguments mslam_hip_match_guided_knn2 and mslam_hip_match_guided share; 0 = go on, 1 = nothing to do (OK)
int guided_check(mslam_hip_ctx* c, const char* who, const uint8_t* kp_desc, const float* kp_xy, int n_kp, const uint8_t* lm_desc,
                 const double* lm_world, int n_lm, const double* R, const double* t, double fx, double fy, int width, int height,
                 double radius)
{
    const std::string me = who;
    if(n_kp < 0 || n_lm < 0 || (n_kp > 0 && (!kp_desc || !kp_xy)) || (n_lm > 0 && (!lm_desc || !lm_world)) || !R || !t)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": bad argument");
    if(n_kp > 65535 || n_lm > 65535)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": more than 65535 keypoints or landmarks are not supported");
    if(!(radius > 0.0))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": the radius is not a positive number");
    if(bad_extent(width) || bad_extent(height))
        return fail(c, MSLAM_HIP_E_INVALID, me + ": the frame extent lies outside 1..8192");
    if(!(fx != 0.0) || !(fy != 0.0) || fx != fx || fy != fy)
        return fail(c, MSLAM_HIP_E_INVALID, me + ": fx or fy is zero or NaN");
    return MSLAM_HIP_OK;
}

// where one host-pointer call's arrays lie: the upload block and the arena
struct GuidedHost
{
    size_t u_xy, u_lm, u_world, up;
    size_t a_off, a_list, a_ldesc, a_idx0, a_idx1, a_dist0, a_dist1, a_ncand, arena;
};

GuidedHost guided_host_layout(int n_kp, int n_lm)
{
    const size_t k = (size_t)std::max(n_kp, 1), l = (size_t)std::max(n_lm, 1);
    GuidedHost h{};
    h.u_xy = al256(k * 32), h.u_lm = h.u_xy + al256(k * 8), h.u_world = h.u_lm + al256(l * 32), h.up = h.u_world + al256(l * 24);
    h.a_off = 0, h.a_list = al256((size_t)(kGuidedMaxCells + 1) * 4), h.a_ldesc = h.a_list + al256(k * 16);
    h.a_idx0 = h.a_ldesc + al256(k * 32);
    h.a_idx1 = h.a_idx0 + al256(l * 4), h.a_dist0 = h.a_idx1 + al256(l * 4), h.a_dist1 = h.a_dist0 + al256(l * 4);
    h.a_ncand = h.a_dist1 + al256(l * 4), h.arena = h.a_ncand + al256(l * 4);
    return h;
}

// upload, bin and knn-2 of one host-pointer call, enqueued on c->stream; the outputs stay in the arena
int guided_host_enqueue(mslam_hip_ctx* c, const GuidedHost& h, const uint8_t* kp_desc, const float* kp_xy, int n_kp,
                        const uint8_t* lm_desc, const double* lm_world, int n_lm, const double* R, const double* t, double fx,
                        double fy, double cx, double cy, int width, int height, double radius, GuidedArgs* out)
{
    RelocState* r = c->reloc;
    if(n_kp > 0)
    {
        std::memcpy(r->h_up, kp_desc, (size_t)n_kp * 32);
        std::memcpy(r->h_up + h.u_xy, kp_xy, (size_t)n_kp * 8);
    }
    std::memcpy(r->h_up + h.u_lm, lm_desc, (size_t)n_lm * 32);
    std::memcpy(r->h_up + h.u_world, lm_world, (size_t)n_lm * 24);
    hipStream_t s = c->stream;
    MSLAM_CHK(c, hipMemcpyAsync(r->d_up, r->h_up, h.up, hipMemcpyHostToDevice, s));
    uint8_t* A = r->d_arena;
    GuidedArgs g{};
    g.kp_desc = r->d_up, g.kp_xy = reinterpret_cast<const float*>(r->d_up + h.u_xy);
    g.n_kp_fixed = n_kp, g.kp_cap = std::max(n_kp, 1);
    g.lm_desc = r->d_up + h.u_lm, g.n_lm_fixed = n_lm, g.cap = n_lm;
    g.world = reinterpret_cast<const double*>(r->d_up + h.u_world);
    std::memcpy(g.R, R, sizeof(g.R));
    std::memcpy(g.t, t, sizeof(g.t));
    g.fx = fx, g.fy = fy, g.cx = cx, g.cy = cy, g.radius = radius;
    g.width = width, g.height = height, g.grid = guided_grid(width, height);
    g.cell_off = reinterpret_cast<int32_t*>(A + h.a_off), g.list = reinterpret_cast<float4*>(A + h.a_list);
    g.list_desc = A + h.a_ldesc;
    g.idx0 = reinterpret_cast<int32_t*>(A + h.a_idx0), g.idx1 = reinterpret_cast<int32_t*>(A + h.a_idx1);
    g.dist0 = reinterpret_cast<int32_t*>(A + h.a_dist0), g.dist1 = reinterpret_cast<int32_t*>(A + h.a_dist1);
    g.n_cand = reinterpret_cast<int32_t*>(A + h.a_ncand);
    {
        StageScope ts(c, "guided_bin");
        launch_guided_bin(g, 1, s);
    }
    {
        StageScope ts(c, "match_guided");
        launch_match_guided(g, 1, s);
    }
    c->last_match_kernel = 3;
    MSLAM_CHK(c, hipGetLastError());
    *out = g;
    return MSLAM_HIP_OK;
}
} // namespace

extern "C" {

int mslam_hip_match_guided_knn2(mslam_hip_ctx* c, const uint8_t* kp_desc, const float* kp_xy, int n_kp, const uint8_t* lm_desc,
                                const double* lm_world, int n_lm, const double* R, const double* t, double fx, double fy, double cx,
                                double cy, int width, int height, double radius, int32_t* idx0, int32_t* idx1, int32_t* dist0,
                                int32_t* dist1, int32_t* n_cand)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    rc = guided_check(c, "match_guided_knn2", kp_desc, kp_xy, n_kp, lm_desc, lm_world, n_lm, R, t, fx, fy, width, height, radius);
    if(rc)
        return rc;
    if(n_lm > 0 && (!idx0 || !idx1 || !dist0 || !dist1))
        return fail(c, MSLAM_HIP_E_INVALID, "match_guided_knn2: bad argument");
    if(n_lm == 0)
        return MSLAM_HIP_OK;
    const GuidedHost h = guided_host_layout(n_kp, n_lm);
    rc = reloc_scratch(c, h.up, h.arena, 16);
    if(rc)
        return rc;
    GuidedArgs g{};
    rc = guided_host_enqueue(c, h, kp_desc, kp_xy, n_kp, lm_desc, lm_world, n_lm, R, t, fx, fy, cx, cy, width, height, radius, &g);
    if(rc)
        return rc;
    const size_t bytes = (size_t)n_lm * 4;
    MSLAM_CHK(c, hipMemcpyAsync(idx0, g.idx0, bytes, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipMemcpyAsync(idx1, g.idx1, bytes, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipMemcpyAsync(dist0, g.dist0, bytes, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipMemcpyAsync(dist1, g.dist1, bytes, hipMemcpyDeviceToHost, c->stream));
    if(n_cand)
        MSLAM_CHK(c, hipMemcpyAsync(n_cand, g.n_cand, bytes, hipMemcpyDeviceToHost, c->stream));
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    return MSLAM_HIP_OK;
}

int mslam_hip_match_guided(mslam_hip_ctx* c, const uint8_t* kp_desc, const float* kp_xy, int n_kp, const uint8_t* lm_desc,
                           const double* lm_world, int n_lm, const double* R, const double* t, double fx, double fy, double cx,
                           double cy, int width, int height, double radius, int max_distance, double ratio, int32_t* from_idx,
                           int32_t* to_idx, int* n_out)
{
    int rc = reloc_enter(c);
    if(rc)
        return rc;
    if(n_out)
        *n_out = 0;
    rc = guided_check(c, "match_guided", kp_desc, kp_xy, n_kp, lm_desc, lm_world, n_lm, R, t, fx, fy, width, height, radius);
    if(rc)
        return rc;
    if(!n_out || (n_lm > 0 && (!from_idx || !to_idx)))
        return fail(c, MSLAM_HIP_E_INVALID, "match_guided: bad argument");
    if(max_distance < 0 || max_distance > 256)
        return fail(c, MSLAM_HIP_E_INVALID, "match_guided: max_distance lies outside 0..256");
    if(n_lm == 0 || n_kp == 0)
        return MSLAM_HIP_OK;
    rc = mslam_ratio_table(c, ratio);
    if(rc)
        return rc;
    const GuidedHost h = guided_host_layout(n_kp, n_lm);
    // the compacted pairs and their count land in the mapped result block: [n, pad | from n_lm | to n_lm]
    rc = reloc_scratch(c, h.up, h.arena, 16 + (size_t)n_lm * 8);
    if(rc)
        return rc;
    RelocState* r = c->reloc;
    GuidedArgs g{};
    rc = guided_host_enqueue(c, h, kp_desc, kp_xy, n_kp, lm_desc, lm_world, n_lm, R, t, fx, fy, cx, cy, width, height, radius, &g);
    if(rc)
        return rc;
    int32_t* h_n = reinterpret_cast<int32_t*>(r->h_res.get());
    h_n[0] = -1; // (overwritten by k_ratio_guided; checked after the synchronisation)
    RatioArgs q{};
    q.idx0 = g.idx0, q.dist0 = g.dist0, q.dist1 = g.dist1;
    q.n_to_fixed = n_lm, q.cap = n_lm;
    q.thr = c->d_ratio_thr;
    q.n_out = reinterpret_cast<int32_t*>(r->h_res.dev());
    q.from_idx = reinterpret_cast<int32_t*>(r->h_res.dev() + 16);
    q.to_idx = q.from_idx + n_lm;
    {
        StageScope ts(c, "ratio_guided");
        launch_ratio_guided(q, max_distance, 1, c->stream);
    }
    MSLAM_CHK(c, hipGetLastError());
    MSLAM_CHK(c, hipStreamSynchronize(c->stream));
    const int32_t n = h_n[0];
    if(n < 0 || n > n_lm)
        return fail(c, MSLAM_HIP_E_RUNTIME, "match_guided: the ratio kernel left no result");
    std::memcpy(from_idx, r->h_res + 16, (size_t)n * 4);
    std::memcpy(to_idx, r->h_res + 16 + (size_t)n_lm * 4, (size_t)n * 4);
    *n_out = n;
    return MSLAM_HIP_OK;
}

int mslam_hip_set_guided_match(mslam_hip_ctx* c, double radius, int max_distance, int width, int height)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(!(radius == radius))
        return fail(c, MSLAM_HIP_E_INVALID, "set_guided_match: the radius is NaN");
    if(max_distance < 0 || max_distance > 256)
        return fail(c, MSLAM_HIP_E_INVALID, "set_guided_match: max_distance lies outside 0..256");
    if(radius > 0.0 && (bad_extent(width) || bad_extent(height)))
        return fail(c, MSLAM_HIP_E_INVALID, "set_guided_match: the frame extent lies outside 1..8192");
    c->guided_radius = radius > 0.0 ? radius : 0.0;
    c->guided_max_distance = max_distance;
    c->guided_width = width, c->guided_height = height;
    return MSLAM_HIP_OK;
}

int mslam_hip_get_guided_match(mslam_hip_ctx* c, double* radius, int* max_distance, int* width, int* height)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(radius)
        *radius = c->guided_radius;
    if(max_distance)
        *max_distance = c->guided_max_distance;
    if(width)
        *width = c->guided_width;
    if(height)
        *height = c->guided_height;
    return MSLAM_HIP_OK;
}

} // extern "C"
