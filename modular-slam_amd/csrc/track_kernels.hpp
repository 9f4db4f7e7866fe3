// track_kernels.hpp — the device code k_track.hip (one frame) and k_track_window.hip (a window of frames) share: the
// vote over one stored keyframe and the construction of a new keyframe's entry, each as the body of one workgroup, so
// that both entry points run the same instructions on the same operands.
#pragma once
#include "reloc.hpp"

namespace mslam
{

// what the step's kernels leave in the call's mapped result block, followed by counts[64], entry_src[K], entry_kp[K]
struct TrackRes
{
    int32_t n_entry, n_inherited, vote_best, vote_best_count;
};

struct VoteCam
{
    double fx, fy, cx, cy, w, h; // w, h = (double)(float)width / height: the reference compares against Vector2f's casts
};

// tracked <=> enough correspondences and a model; ncorr == nullptr (mslam_hip_kf_visible): the record alone decides
__device__ __forceinline__ bool track_ok(const double* __restrict__ rec, const int32_t* __restrict__ ncorr, int min_matched)
{
    return rec[14] == 1.0 && (!ncorr || *ncorr >= min_matched);
}

// One workgroup (256 threads) and one listed keyframe, lanes strided over its landmarks: how many of them project into
// the frame whose pose record is `rec`.
__device__ __forceinline__ void track_vote_block(const double* __restrict__ store_world, const int32_t* __restrict__ store_n,
                                                 int slot, int K, const double* __restrict__ rec,
                                                 const int32_t* __restrict__ ncorr, int min_matched, const VoteCam& cam,
                                                 int32_t* __restrict__ count)
{
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if(!track_ok(rec, ncorr, min_matched))
    {
        if(tid == 0)
            *count = 0;
        return;
    }
    const int n = min(max(store_n[slot], 0), K);
    const double* world = store_world + (size_t)slot * K * 3;
    uint32_t mine = 0; // (wave-uniform: every lane adds the same popcount)
    for(int base = 0; base < n; base += 256)
    {
        const int i = base + tid;
        bool vis = false;
        if(i < n)
        {
            const double X = world[3 * (size_t)i], Y = world[3 * (size_t)i + 1], Z = world[3 * (size_t)i + 2];
            const double c0 = ((rec[0] * X + rec[1] * Y) + rec[2] * Z) + rec[9];
            const double c1 = ((rec[3] * X + rec[4] * Y) + rec[5] * Z) + rec[10];
            const double c2 = ((rec[6] * X + rec[7] * Y) + rec[8] * Z) + rec[11];
            const double u = (c0 / c2) * cam.fx + cam.cx, v = (c1 / c2) * cam.fy + cam.cy;
            vis = u >= 0.0 && u < cam.w && v >= 0.0 && v < cam.h && c2 > 0.0;
        }
        mine += (uint32_t)__popcll(__ballot(vis));
    }
    if(lane == 0)
        wsum[wave] = mine;
    __syncthreads();
    if(tid == 0)
        *count = (int32_t)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

struct KeyframeArgs
{
    // the step's outputs for the one candidate (row 0)
    const int32_t *mfrom, *mto, *mcount, *g_cnt, *ncorr;
    const uint8_t* mask;
    const double* rec;
    int min_matched, kf_min_landmarks;
    // the query
    const uint8_t* desc;
    const double* xyz;
    const uint8_t* valid;
    int nq, S;
    double z_max;
    // the store: the reference entry's world points and landmark ids, the new entry's slot
    const double* ref_world;
    const int64_t* ref_lid;
    uint8_t* out_desc;
    double* out_world;
    int64_t* out_lid;
    int64_t lid_base; // landmark o of part B gets the fresh id lid_base | o
    int32_t* out_n;
    int cap;
    // mapped host block
    TrackRes* h_res;
    int32_t *h_src, *h_kp;
};

// One workgroup builds the new keyframe's entry in its store slot.  Part A: the inlier correspondences in correspondence
// order, with the reference entry's world points and landmark ids copied bit for bit.  Part B: every keypoint no correspondence used, with a
// valid depth and z <= z_max, in keypoint order, lifted with world = R^T (p - t).  Ordered ballot / prefix compaction as
// k_kf_lift.  nq <= 65536 (the host checks nq <= cap <= 65535).  There is one match per reference landmark, so two
// landmarks can name the same keypoint and part A then lists it twice: A and B together can exceed nq, and every store
// is guarded by o < cap (the entry is cut at cap, part A first).
__device__ __forceinline__ void track_keyframe_block(const KeyframeArgs& a)
{
    __shared__ uint32_t used[2048];
    __shared__ uint32_t wsum[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* rec = a.rec;
    if(!track_ok(rec, a.ncorr, a.min_matched) || (int)rec[12] >= a.kf_min_landmarks)
        return; // not tracked, or no keyframe required: the slot and the (pre-zeroed) result stay as they are
    for(int i = tid; i < 2048; i += 256)
        used[i] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const int m = min(max(a.mcount[0], 0), a.S), n_to = a.g_cnt[0];
    uint32_t run_c = 0, run_a = 0; // correspondences / part A entries so far
    for(int base = 0; base < m; base += 256)
    {
        const int i = base + tid;
        int from = 0, to = 0;
        bool ok = false; // k_reloc_corr's own condition: the j-th `ok` match is correspondence j
        if(i < m)
        {
            from = a.mfrom[i], to = a.mto[i];
            ok = (unsigned)from < (unsigned)a.nq && (unsigned)to < (unsigned)n_to && a.valid[from] != 0;
        }
        const unsigned long long bc = __ballot(ok);
        if(lane == 0)
            wsum[0][wave] = (uint32_t)__popcll(bc);
        __syncthreads();
        uint32_t pre_c = 0, tot_c = 0;
        for(int k = 0; k < 4; ++k)
        {
            pre_c += k < wave ? wsum[0][k] : 0;
            tot_c += wsum[0][k];
        }
        bool inl = false;
        if(ok)
        {
            atomicOr(&used[from >> 5], 1u << (from & 31)); // used = matched with a valid depth, inlier or not (:314-334)
            inl = a.mask[run_c + pre_c + (uint32_t)__popcll(bc & below)] != 0;
        }
        const unsigned long long ba = __ballot(inl);
        if(lane == 0)
            wsum[1][wave] = (uint32_t)__popcll(ba);
        __syncthreads();
        uint32_t pre_a = 0, tot_a = 0;
        for(int k = 0; k < 4; ++k)
        {
            pre_a += k < wave ? wsum[1][k] : 0;
            tot_a += wsum[1][k];
        }
        const size_t o = run_a + pre_a + (uint32_t)__popcll(ba & below);
        if(inl && o < (size_t)a.cap)
        {
            copy_desc(a.desc + (size_t)from * 32, a.out_desc + o * 32);
            const double* P = a.ref_world + (size_t)to * 3;
            a.out_world[o * 3] = P[0], a.out_world[o * 3 + 1] = P[1], a.out_world[o * 3 + 2] = P[2];
            a.out_lid[o] = a.ref_lid[to];
            a.h_src[o] = to, a.h_kp[o] = from;
        }
        run_c += tot_c;
        run_a += tot_a;
        __syncthreads(); // wsum is rewritten by the next round; after the last round: the bitmap is complete
    }
    const uint32_t n_a = min(run_a, (uint32_t)a.cap);
    const double t0 = rec[9], t1 = rec[10], t2 = rec[11];
    uint32_t run = n_a;
    for(int base = 0; base < a.nq; base += 256)
    {
        const int i = base + tid;
        bool ok = false;
        double x = 0, y = 0, z = 0;
        if(i < a.nq && !((used[i >> 5] >> (i & 31)) & 1u) && a.valid[i] != 0)
        {
            x = a.xyz[3 * (size_t)i], y = a.xyz[3 * (size_t)i + 1], z = a.xyz[3 * (size_t)i + 2];
            ok = z <= a.z_max;
        }
        const unsigned long long b = __ballot(ok);
        if(lane == 0)
            wsum[0][wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for(int k = 0; k < 4; ++k)
        {
            pre += k < wave ? wsum[0][k] : 0;
            tot += wsum[0][k];
        }
        const size_t o = run + pre + (uint32_t)__popcll(b & below);
        if(ok && o < (size_t)a.cap)
        {
            copy_desc(a.desc + (size_t)i * 32, a.out_desc + o * 32);
            const double dx = x - t0, dy = y - t1, dz = z - t2;
            a.out_world[o * 3] = (rec[0] * dx + rec[3] * dy) + rec[6] * dz; // R^T (p - t): column r of R
            a.out_world[o * 3 + 1] = (rec[1] * dx + rec[4] * dy) + rec[7] * dz;
            a.out_world[o * 3 + 2] = (rec[2] * dx + rec[5] * dy) + rec[8] * dz;
            a.out_lid[o] = a.lid_base | (int64_t)o;
            a.h_src[o] = -1, a.h_kp[o] = i;
        }
        run += tot;
        __syncthreads();
    }
    if(tid == 0)
    {
        const int32_t n_entry = (int32_t)min(run, (uint32_t)a.cap);
        *a.out_n = n_entry;
        a.h_res->n_entry = n_entry;
        a.h_res->n_inherited = (int32_t)n_a;
    }
}

} // namespace mslam
