// k_tsdf_raycast.hip — the view of the dense TSDF map from a pose: mslam_hip_tsdf_raycast (include/mslam_hip.h has the per-pixel
// rule; DESIGN.md 4.33 the structure).  One thread per pixel, a wave owns an 8 x 8 pixel tile (neighbouring rays read
// neighbouring voxels), a workgroup 2 x 2 of them.  Every pixel is computed from the volume alone, in f64, one separately
// rounded operation after the other: no atomics, nothing shared between pixels, so the images have one value, bit for bit.
//   k_tsdf_raycast   per ray: a conservative clip of the sample range against the volume's box, then the march as a state
//                    machine with ONE field evaluation per iteration (the lanes of a wave stay together on the eight 8-byte
//                    (S, W) loads whatever step of the rule each of them is in), the hit point, six more evaluations for the
//                    normal of a hit.  The hits of a workgroup are counted by ballot in a fixed order.
#include "context.hpp"
#include "tsdf.hpp"
#include <cmath>
#include <cstring>
#include <vector>

namespace mslam
{

constexpr int kRayTile = 8;                  // a wave: 8 x 8 pixels
constexpr int kRayBlock = 2 * kRayTile;      // a workgroup: 16 x 16 pixels, wave w at (w & 1, w >> 1)
constexpr int kRayThreads = 256;
static_assert(kRayTile * kRayTile == 64 && kRayBlock * kRayBlock == kRayThreads, "tile shape");

struct TsdfRayArgs
{
    const int2* vol;
    int nx, ny, nz;
    double voxel, ox, oy, oz;
    int width, height;
    unsigned tiles_x; // workgroups per row of 16 x 16 tiles
    double fx, fy, cx, cy;
    double R[9], t[3];
    double z_near, step;
    int n_last, K, min_weight; // K <= n_last + 1: every larger stride walks all samples, as n_last + 1 does
    float* depth;              // [height][width]
    float* xyz;                // [height][width][3] or nullptr
    float* normal;             // [height][width][3] or nullptr
    unsigned* block_hits;      // [workgroups]
};

struct TsdfSample
{
    double F;
    bool valid;
};

// F(P) of the rule.  A sample that is not valid reads nothing beyond the corners' own voxels: the index test comes first.
__device__ __forceinline__ TsdfSample tsdf_field(const TsdfRayArgs& a, double Px, double Py, double Pz)
{
    TsdfSample s{0.0, false};
    const double gx = (Px - a.ox) / a.voxel - 0.5, gy = (Py - a.oy) / a.voxel - 0.5, gz = (Pz - a.oz) / a.voxel - 0.5;
    const double bx = floor(gx), by = floor(gy), bz = floor(gz);
    if(!(bx >= 0.0 && bx + 1.0 <= (double)(a.nx - 1) && by >= 0.0 && by + 1.0 <= (double)(a.ny - 1) && bz >= 0.0 &&
         bz + 1.0 <= (double)(a.nz - 1))) // false for NaN
        return s;
    const double wx = gx - bx, wy = gy - by, wz = gz - bz;
    // 0 <= b and b + 1 <= n - 1: all eight corners are voxels of the volume
    const size_t row = (size_t)a.nx, slab = (size_t)a.nx * (size_t)a.ny;
    const int2* p = a.vol + (((size_t)(int)bz * (size_t)a.ny + (size_t)(int)by) * row + (size_t)(int)bx);
    const int2 c000 = p[0], c100 = p[1], c010 = p[row], c110 = p[row + 1];
    const int2 c001 = p[slab], c101 = p[slab + 1], c011 = p[slab + row], c111 = p[slab + row + 1];
    const int w = a.min_weight; // >= 1: no division by zero below
    if(c000.y < w || c100.y < w || c010.y < w || c110.y < w || c001.y < w || c101.y < w || c011.y < w || c111.y < w)
        return s;
    const double v000 = (double)c000.x / (double)c000.y, v100 = (double)c100.x / (double)c100.y;
    const double v010 = (double)c010.x / (double)c010.y, v110 = (double)c110.x / (double)c110.y;
    const double v001 = (double)c001.x / (double)c001.y, v101 = (double)c101.x / (double)c101.y;
    const double v011 = (double)c011.x / (double)c011.y, v111 = (double)c111.x / (double)c111.y;
    const double x00 = v000 + wx * (v100 - v000), x10 = v010 + wx * (v110 - v010);
    const double x01 = v001 + wx * (v101 - v001), x11 = v011 + wx * (v111 - v011);
    const double y0 = x00 + wy * (x10 - x00), y1 = x01 + wy * (x11 - x01);
    s.F = y0 + wz * (y1 - y0);
    s.valid = true;
    return s;
}

__device__ __forceinline__ bool tsdf_near(const TsdfSample& s) { return s.valid && s.F < 32767.0; }

// The samples [n_lo, n_hi] outside which the rule makes every sample of the ray invalid; n_lo > n_hi: none can be valid.
// A valid sample has 0 <= floor(g_a) and floor(g_a) + 1 <= n_a - 1 on every axis, so in exact arithmetic P_a lies in the slab
// [o_a + 0.5 voxel, o_a + (n_a - 0.5) voxel).  The computed P_a and g_a differ from the exact ones by a few 2^-53 of
// mag_a = |C_a| + z_end |D_a| + |o_a| + n_a voxel (the magnitudes that enter the sums), and so does the numerator of the
// slab's crossing (bound - C_a).  The slab is widened by delta_a = 1e-9 mag_a on both sides: more than 10^6 times those
// errors, whatever |D_a| divides them by, so a near-parallel ray (tiny |D_a|) is safe too.  What is left is the rounding of
// the two quotients that turn a crossing into a sample number, below 2^-50 of a number that is below 2^21 where it matters,
// and of z_n itself (below 2^-31 samples): one sample of slack on either side covers them (floor - 1, floor + 2).
// D_a == 0 puts no bound on that axis (the ray is parallel to the faces: kept), and every comparison is written so that a
// NaN keeps the ray.
__device__ __forceinline__ void tsdf_ray_clip(const TsdfRayArgs& a, const double C[3], const double D[3], int& n_lo, int& n_hi)
{
    n_lo = 0, n_hi = a.n_last;
    const double z_end = a.z_near + (double)a.n_last * a.step;
    const double o[3] = {a.ox, a.oy, a.oz};
    const int nn[3] = {a.nx, a.ny, a.nz};
    for(int e = 0; e < 3; ++e)
    {
        if(!(D[e] > 0.0 || D[e] < 0.0))
            continue;
        const double ext = (double)nn[e] * a.voxel;
        const double delta = 1e-9 * (((fabs(C[e]) + z_end * fabs(D[e])) + fabs(o[e])) + ext);
        const double lo = (o[e] + 0.5 * a.voxel) - delta, hi = (o[e] + ((double)nn[e] - 0.5) * a.voxel) + delta;
        double t0 = (lo - C[e]) / D[e], t1 = (hi - C[e]) / D[e];
        if(t0 > t1)
        {
            const double s = t0;
            t0 = t1, t1 = s;
        }
        const double x = floor((t0 - a.z_near) / a.step) - 1.0, y = floor((t1 - a.z_near) / a.step) + 2.0;
        if(x > (double)n_lo)
            n_lo = x > (double)a.n_last ? a.n_last + 1 : (int)x;
        if(y < (double)n_hi)
            n_hi = y < 0.0 ? -1 : (int)y;
    }
}

__global__ __launch_bounds__(kRayThreads) void k_tsdf_raycast(const TsdfRayArgs a)
{
    __shared__ int s_wave[kRayThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
    const int px = (int)bx * kRayBlock + (wave & 1) * kRayTile + (lane & (kRayTile - 1));
    const int py = (int)by * kRayBlock + (wave >> 1) * kRayTile + (lane >> 3);
    const bool inside = px < a.width && py < a.height;

    double C[3], D[3];
    const double dx = ((double)px - a.cx) / a.fx, dy = ((double)py - a.cy) / a.fy;
    for(int e = 0; e < 3; ++e)
    {
        C[e] = -((a.R[e] * a.t[0] + a.R[3 + e] * a.t[1]) + a.R[6 + e] * a.t[2]);
        D[e] = (a.R[e] * dx + a.R[3 + e] * dy) + a.R[6 + e];
    }
    int n_lo, n_hi;
    tsdf_ray_clip(a, C, D, n_lo, n_hi);
    // a sample outside the clip is invalid by the rule: it costs nothing
    auto sample = [&](int n) -> TsdfSample {
        if(n < n_lo || n > n_hi)
            return TsdfSample{0.0, false};
        const double z = a.z_near + (double)n * a.step;
        return tsdf_field(a, C[0] + z * D[0], C[1] + z * D[1], C[2] + z * D[2]);
    };

    const int K = a.K;
    bool done = !inside || n_lo > n_hi, hit = false;
    // Every coarse stride that ends at or before n_lo joins two invalid samples and is skipped by the rule, up to the base
    // n = floor(n_lo / K) K <= n_lo.  When that base IS n_lo, its sample may end the ray: sample 0 by the rule's first
    // sentence, a later one because the walk that reaches it comes from invalid samples.  Either way a miss.
    int n = 0, m = 0, m_hit = 0;
    double F0 = 0.0, F1 = 0.0;
    TsdfSample sn{0.0, false}, sc{0.0, false}, prev{0.0, false};
    if(!done)
    {
        n = (n_lo / K) * K;
        sn = sample(n);
        if(sn.valid && sn.F <= 0.0)
            done = true;
    }
    bool walking = false, have_c = false;
    while(!done) // a lane leaves when its ray has ended; the wave when all have
    {
        int idx = -1;
        if(!walking)
        {
            if(n > n_hi) // this sample and all later ones are invalid
            {
                done = true;
                continue;
            }
            if(n + K <= a.n_last)
                idx = n + K;
            else
            {
                walking = true, have_c = false, m = n + 1, prev = sn;
                continue;
            }
        }
        else
        {
            if(m > a.n_last)
            {
                done = true;
                continue;
            }
            if(!(have_c && m == n + K))
                idx = m;
        }
        const TsdfSample cur = idx >= 0 ? sample(idx) : sc;
        if(!walking)
        {
            sc = cur;
            if(!tsdf_near(sn) && !tsdf_near(sc))
                n += K, sn = sc;
            else
                walking = true, have_c = true, m = n + 1, prev = sn;
        }
        else if(cur.valid && cur.F <= 0.0)
        {
            done = true;
            if(prev.valid)
                hit = true, m_hit = m, F0 = prev.F, F1 = cur.F;
        }
        else
        {
            prev = cur;
            if(++m > n + K)
                n += K, sn = prev, walking = false;
        }
    }

    float o_depth = 0.f, o_xyz[3] = {0.f, 0.f, 0.f}, o_n[3] = {0.f, 0.f, 0.f};
    if(hit)
    {
        const double zs = (a.z_near + (double)(m_hit - 1) * a.step) + (F0 / (F0 - F1)) * a.step;
        const double P[3] = {C[0] + zs * D[0], C[1] + zs * D[1], C[2] + zs * D[2]};
        o_depth = (float)zs;
        for(int e = 0; e < 3; ++e)
            o_xyz[e] = (float)P[e];
        if(a.normal)
        {
            const TsdfSample xp = tsdf_field(a, P[0] + a.voxel, P[1], P[2]), xm = tsdf_field(a, P[0] - a.voxel, P[1], P[2]);
            const TsdfSample yp = tsdf_field(a, P[0], P[1] + a.voxel, P[2]), ym = tsdf_field(a, P[0], P[1] - a.voxel, P[2]);
            const TsdfSample zp = tsdf_field(a, P[0], P[1], P[2] + a.voxel), zm = tsdf_field(a, P[0], P[1], P[2] - a.voxel);
            if(xp.valid && xm.valid && yp.valid && ym.valid && zp.valid && zm.valid)
            {
                const double hx = xp.F - xm.F, hy = yp.F - ym.F, hz = zp.F - zm.F;
                const double len = sqrt((hx * hx + hy * hy) + hz * hz);
                if(len > 0.0)
                    o_n[0] = (float)(hx / len), o_n[1] = (float)(hy / len), o_n[2] = (float)(hz / len);
            }
        }
    }
    if(inside)
    {
        const size_t pix = (size_t)py * (size_t)a.width + (size_t)px;
        a.depth[pix] = o_depth;
        for(int e = 0; e < 3; ++e)
        {
            if(a.xyz)
                a.xyz[pix * 3 + e] = o_xyz[e];
            if(a.normal)
                a.normal[pix * 3 + e] = o_n[e];
        }
    }
    const int hits = __popcll(__ballot(hit));
    if(lane == 0)
        s_wave[wave] = hits;
    __syncthreads();
    if(threadIdx.x == 0)
        a.block_hits[blockIdx.x] = (unsigned)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static bool ray_finite(const double* v, int n)
{
    for(int i = 0; i < n; ++i)
        if(!std::isfinite(v[i]))
            return false;
    return true;
}

static int tsdf_raycast(mslam_hip_ctx* c, const mslam_hip_tsdf_raycast_params* p, const double* R, const double* t, float* depth,
                        float* xyz, float* normal, int* n_hits, bool to_device, const char* who)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": no volume (mslam_hip_tsdf_create)");
    if(!p || !R || !t || !depth)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": NULL params, R, t or depth");
    if(p->width < 1 || p->height < 1 || (long long)p->width * p->height > (1 << 30))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": width, height must be >= 1 with at most 2^30 pixels");
    if(!(p->fx != 0) || !(p->fy != 0) || std::isnan(p->fx) || std::isnan(p->fy))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": a focal length of zero or NaN");
    if(!std::isfinite(p->cx) || !std::isfinite(p->cy) || !ray_finite(R, 9) || !ray_finite(t, 3))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": a non-finite cx, cy, R or t");
    if(!std::isfinite(p->z_near) || p->z_near < 0 || !std::isfinite(p->z_far) || p->z_far < p->z_near)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": z_near must be finite and >= 0, z_far finite and >= z_near");
    if(!std::isfinite(p->step) || !(p->step > 0) || !((p->z_far - p->z_near) / p->step < (double)(1 << 20)))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": step must be finite and > 0 with fewer than 2^20 samples");
    if(p->coarse < 1 || p->min_weight < 1)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": coarse and min_weight must be >= 1");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": hipSetDevice");

    TsdfRayArgs a{};
    a.vol = s->vol;
    a.nx = s->p.nx, a.ny = s->p.ny, a.nz = s->p.nz;
    a.voxel = s->p.voxel, a.ox = s->p.origin[0], a.oy = s->p.origin[1], a.oz = s->p.origin[2];
    a.width = p->width, a.height = p->height;
    a.fx = p->fx, a.fy = p->fy, a.cx = p->cx, a.cy = p->cy;
    std::memcpy(a.R, R, sizeof(a.R));
    std::memcpy(a.t, t, sizeof(a.t));
    a.z_near = p->z_near, a.step = p->step;
    // the last n with z_n <= z_far: the quotient is within a sample of it
    int n_last = (int)std::floor((p->z_far - p->z_near) / p->step);
    while(p->z_near + (double)(n_last + 1) * p->step <= p->z_far)
        ++n_last;
    while(n_last > 0 && p->z_near + (double)n_last * p->step > p->z_far)
        --n_last;
    a.n_last = n_last;
    a.K = std::min(p->coarse, n_last + 1);
    a.min_weight = p->min_weight;
    a.tiles_x = (unsigned)((p->width + kRayBlock - 1) / kRayBlock);
    // <= 2^30 pixels: at most 2^26 + 1 workgroups even for an image one pixel high
    const unsigned n_blocks = a.tiles_x * (unsigned)((p->height + kRayBlock - 1) / kRayBlock);
    const size_t px = (size_t)p->width * (size_t)p->height;

    hipError_t e = grow(s->d_ray_hits, n_blocks, c->stream);
    a.block_hits = s->d_ray_hits;
    if(to_device)
        a.depth = depth, a.xyz = xyz, a.normal = normal;
    else
    {
        if(e == hipSuccess)
            e = grow(s->d_ray_depth, px, c->stream);
        if(e == hipSuccess && xyz)
            e = grow(s->d_xyz, px * 3, c->stream);
        if(e == hipSuccess && normal)
            e = grow(s->d_normal, px * 3, c->stream);
        a.depth = s->d_ray_depth, a.xyz = xyz ? s->d_xyz.get() : nullptr, a.normal = normal ? s->d_normal.get() : nullptr;
    }
    if(e == hipSuccess)
    {
        StageScope ts(c, "tsdf_raycast");
        hipLaunchKernelGGL(k_tsdf_raycast, dim3(n_blocks), dim3(kRayThreads), 0, c->stream, a);
        e = hipGetLastError();
    }
    if(!to_device)
    {
        if(e == hipSuccess)
            e = hipMemcpyAsync(depth, a.depth, px * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if(e == hipSuccess && xyz)
            e = hipMemcpyAsync(xyz, a.xyz, px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if(e == hipSuccess && normal)
            e = hipMemcpyAsync(normal, a.normal, px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    std::vector<unsigned> counts;
    if(e == hipSuccess && n_hits)
    {
        counts.resize(n_blocks);
        e = hipMemcpyAsync(counts.data(), a.block_hits, (size_t)n_blocks * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    }
    if(e == hipSuccess && (!to_device || n_hits))
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": " + hipGetErrorString(e));
    if(n_hits)
    {
        unsigned long long total = 0; // in index order
        for(unsigned v : counts)
            total += v;
        *n_hits = (int)total;
    }
    return MSLAM_HIP_OK;
}

} // namespace mslam

using namespace mslam;

extern "C" int mslam_hip_tsdf_raycast(mslam_hip_ctx* c, const mslam_hip_tsdf_raycast_params* p, const double* R, const double* t,
                                      float* depth, float* xyz, float* normal, int* n_hits)
{
    return tsdf_raycast(c, p, R, t, depth, xyz, normal, n_hits, false, "tsdf_raycast");
}

extern "C" int mslam_hip_tsdf_raycast_dev(mslam_hip_ctx* c, const mslam_hip_tsdf_raycast_params* p, const double* R,
                                          const double* t, float* d_depth, float* d_xyz, float* d_normal, int* n_hits)
{
    return tsdf_raycast(c, p, R, t, d_depth, d_xyz, d_normal, n_hits, true, "tsdf_raycast_dev");
}
