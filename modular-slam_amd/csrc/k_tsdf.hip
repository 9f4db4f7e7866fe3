// k_tsdf.hip — the dense TSDF map of mslam_hip_tsdf_* (include/mslam_hip.h has the per-voxel rule and the extraction rule;
// DESIGN.md 4.32 the structure).  Integer accumulators (S, W) per voxel make integrating a frame an exact add and taking it
// out again the exact inverse, so the volume can follow the keyframe poses the back end corrects.
//   k_tsdf_sweep         one pass over the volume applies up to MSLAM_HIP_TSDF_CHUNK (frame, sign) entries: a wave owns a
//                        16 x 4 x 1 tile of voxels, lane f tests entry f against the tile (behind the camera, beyond
//                        max_depth + trunc, beside the frustum), a ballot makes the survivors a wave-uniform bit mask, and
//                        every voxel walks that mask.  One 8-byte load and at most one 8-byte store per voxel and sweep.
//   k_tsdf_count / k_tsdf_scan / k_tsdf_write   surface points in index order: crossings per workgroup, an exclusive scan,
//                        then every workgroup writes at its offset.
#include "context.hpp"
#include "tsdf.hpp"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

namespace mslam
{

void tsdf_destroy(TsdfState* s) { delete s; }

constexpr int kTsdfTx = 16, kTsdfTy = 4, kTsdfTz = 4; // a wave: 16 x 4 x 1 voxels; a workgroup: 4 waves stacked along z
constexpr int kTsdfThreads = 256;
constexpr int kTsdfMaxBlocks = 2048; // the sweep walks its tiles with a grid stride
static_assert(MSLAM_HIP_TSDF_CHUNK == 64, "lane f of a wave tests entry f of the chunk");
static_assert(kTsdfTx * kTsdfTy == 64 && kTsdfTz * 64 == kTsdfThreads, "tile shape");

struct TsdfSweepArgs
{
    int2* vol;
    int nx, ny, nz;
    unsigned tiles_x, tiles_y, n_tiles;
    double voxel, ox, oy, oz, trunc, max_depth;
    int width, height;
    float factor;
    double fx, fy, cx, cy;
    const TsdfEntry* e; // this chunk's entries
    int n;              // 1..MSLAM_HIP_TSDF_CHUNK
};

// May entry e change a voxel whose centre lies in the box (Xc +- hx, Yc +- hy, Zc)?  false only when the rule provably skips
// every such voxel.  The camera-space box is the centre's image +- |R| (hx, hy, 0), widened by 1e-12 of the magnitudes that
// enter the sums (the per-voxel sums differ from the exact ones by a few 2^-53 of the same magnitudes), so that it holds the
// COMPUTED c_r of every voxel; the tests on it are the rule's own comparisons, made conservative.  Every test is written so
// that a NaN keeps the entry.
__device__ __forceinline__ bool tsdf_entry_reaches(const TsdfSweepArgs& a, const TsdfEntry& e, double Xc, double Yc, double Zc,
                                                   double hx, double hy)
{
    double cm[3], ex[3], am[3];
    for(int r = 0; r < 3; ++r)
    {
        const double r0 = e.R[3 * r], r1 = e.R[3 * r + 1], r2 = e.R[3 * r + 2];
        cm[r] = ((r0 * Xc + r1 * Yc) + r2 * Zc) + e.t[r];
        const double mag = ((fabs(r0) * (fabs(Xc) + hx) + fabs(r1) * (fabs(Yc) + hy)) + fabs(r2) * fabs(Zc)) + fabs(e.t[r]);
        ex[r] = (fabs(r0) * hx + fabs(r1) * hy) + 1e-12 * mag;
        am[r] = fabs(cm[r]) + ex[r];
    }
    const double lo2 = cm[2] - ex[2], hi2 = cm[2] + ex[2];
    if(hi2 <= 0.0)
        return false; // c_2 > 0 fails everywhere
    // d <= max_depth and c_2 >= lo2 give d - c_2 <= max_depth - lo2, and rounding is monotone
    if(a.max_depth - lo2 < -a.trunc)
        return false;
    // uh < 0 <=> fx c_0 + (cx + 0.5) c_2 < 0 (c_2 > 0); the computed uh differs from the exact one by a few 2^-53 of
    // |c_0 / c_2 fx| + |cx| + 0.5, and a quotient that underflows by less than 2^-1022: both inside the slack
    const double bl = a.cx + 0.5, br = bl - (double)a.width;
    const double sl_u = 1e-12 * (fabs(a.fx) * am[0] + (fabs(a.cx) + 0.5 + (double)a.width) * am[2]) + 1e-290 * am[2];
    if((a.fx * cm[0] + bl * cm[2]) + (fabs(a.fx) * ex[0] + fabs(bl) * ex[2]) < -sl_u)
        return false;
    if((a.fx * cm[0] + br * cm[2]) - (fabs(a.fx) * ex[0] + fabs(br) * ex[2]) > sl_u)
        return false; // uh >= width everywhere
    const double bt = a.cy + 0.5, bb = bt - (double)a.height;
    const double sl_v = 1e-12 * (fabs(a.fy) * am[1] + (fabs(a.cy) + 0.5 + (double)a.height) * am[2]) + 1e-290 * am[2];
    if((a.fy * cm[1] + bt * cm[2]) + (fabs(a.fy) * ex[1] + fabs(bt) * ex[2]) < -sl_v)
        return false;
    if((a.fy * cm[1] + bb * cm[2]) - (fabs(a.fy) * ex[1] + fabs(bb) * ex[2]) > sl_v)
        return false;
    return true;
}

__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_sweep(const TsdfSweepArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for(unsigned tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x)
    {
        const unsigned tx = tile % a.tiles_x, tyz = tile / a.tiles_x;
        const unsigned ty = tyz % a.tiles_y, tz = tyz / a.tiles_y;
        const int i0 = (int)tx * kTsdfTx, j0 = (int)ty * kTsdfTy, k = (int)tz * kTsdfTz + wave;
        if(k >= a.nz) // the whole wave
            continue;
        const int i1 = min(i0 + kTsdfTx - 1, a.nx - 1), j1 = min(j0 + kTsdfTy - 1, a.ny - 1);
        const double Z = a.oz + ((double)k + 0.5) * a.voxel;
        bool reach = false;
        if(lane < a.n)
        {
            const double Xc = a.ox + ((double)(i0 + i1) * 0.5 + 0.5) * a.voxel, Yc = a.oy + ((double)(j0 + j1) * 0.5 + 0.5) * a.voxel;
            // half extents of the centres, a little generous: X of a voxel is itself a rounded sum
            const double hx = (double)(i1 - i0) * 0.5 * a.voxel + 1e-12 * (fabs(Xc) + fabs(a.ox)),
                         hy = (double)(j1 - j0) * 0.5 * a.voxel + 1e-12 * (fabs(Yc) + fabs(a.oy));
            reach = tsdf_entry_reaches(a, a.e[lane], Xc, Yc, Z, hx, hy);
        }
        unsigned long long todo = __ballot(reach);
        const int i = i0 + (lane & (kTsdfTx - 1)), j = j0 + (lane >> 4);
        if(todo == 0 || i >= a.nx || j >= a.ny) // lanes past the volume's edge only took part in the test
            continue;
        const size_t idx = ((size_t)k * (size_t)a.ny + (size_t)j) * (size_t)a.nx + (size_t)i;
        const int2 before = a.vol[idx];
        int S = before.x, W = before.y;
        const double X = a.ox + ((double)i + 0.5) * a.voxel, Y = a.oy + ((double)j + 0.5) * a.voxel;
        while(todo)
        {
            const int f = __ffsll(todo) - 1; // wave-uniform: the entry comes through scalar loads
            todo &= todo - 1;
            const TsdfEntry& e = a.e[f];
            const double c2 = ((e.R[6] * X + e.R[7] * Y) + e.R[8] * Z) + e.t[2];
            if(!(c2 > 0.0))
                continue;
            const double c0 = ((e.R[0] * X + e.R[1] * Y) + e.R[2] * Z) + e.t[0];
            const double c1 = ((e.R[3] * X + e.R[4] * Y) + e.R[5] * Z) + e.t[1];
            const double u = (c0 / c2) * a.fx + a.cx, v = (c1 / c2) * a.fy + a.cy;
            const double uh = u + 0.5, vh = v + 0.5;
            if(!(uh >= 0.0 && uh < (double)a.width && vh >= 0.0 && vh < (double)a.height))
                continue;
            const int px = (int)floor(uh), py = (int)floor(vh); // 0 <= px < width, 0 <= py < height
            const float d = (float)e.depth[py * a.width + px] * a.factor;
            if(!(d > FLT_EPSILON && (double)d <= a.max_depth))
                continue;
            const double sdf = (double)d - c2;
            if(sdf < -a.trunc)
                continue;
            double x = sdf / a.trunc;
            if(x > 1.0)
                x = 1.0;
            const int q = (int)rint(x * 32767.0);
            S += e.sign * q;
            W += e.sign;
        }
        if(S != before.x || W != before.y)
            a.vol[idx] = make_int2(S, W);
    }
}

// ---- extraction -----------------------------------------------------------------------------------------------------------
struct TsdfExtractArgs
{
    const int2* vol;
    int nx, ny, nz;
    size_t n_voxels;
    int min_weight;
    double voxel, ox, oy, oz;
    unsigned long long* block_ofs; // [n_blocks + 1]
    unsigned n_blocks;
    float* xyz;    // [total][3]
    float* normal; // [total][3]
};

// The voxel of thread `idx`: its value, its three forward neighbours (ok[e]: inside and observed), the crossing bits.
struct TsdfCell
{
    int i, j, k;
    int2 a, b[3];
    bool ok[3];
    int cross; // bit e: a crossing along axis e
};
__device__ __forceinline__ TsdfCell tsdf_cell(const TsdfExtractArgs& g, size_t idx)
{
    TsdfCell c{};
    if(idx >= g.n_voxels)
        return c;
    c.i = (int)(idx % (size_t)g.nx);
    const size_t jk = idx / (size_t)g.nx;
    c.j = (int)(jk % (size_t)g.ny);
    c.k = (int)(jk / (size_t)g.ny);
    c.a = g.vol[idx];
    if(c.a.y < g.min_weight)
        return c;
    const bool in[3] = {c.i + 1 < g.nx, c.j + 1 < g.ny, c.k + 1 < g.nz};
    const size_t step[3] = {1, (size_t)g.nx, (size_t)g.nx * (size_t)g.ny};
    for(int e = 0; e < 3; ++e)
    {
        if(!in[e])
            continue;
        c.b[e] = g.vol[idx + step[e]];
        c.ok[e] = c.b[e].y >= g.min_weight;
        if(c.ok[e] && ((c.a.x < 0) != (c.b[e].x < 0)))
            c.cross |= 1 << e;
    }
    return c;
}

__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_count(const TsdfExtractArgs g)
{
    __shared__ int s_wave[kTsdfThreads / 64];
    const TsdfCell c = tsdf_cell(g, (size_t)blockIdx.x * kTsdfThreads + threadIdx.x);
    int n = __popc(c.cross);
    for(int o = 32; o; o >>= 1)
        n += __shfl_xor(n, o);
    if((threadIdx.x & 63) == 0)
        s_wave[threadIdx.x >> 6] = n;
    __syncthreads();
    if(threadIdx.x == 0)
        g.block_ofs[blockIdx.x] = (unsigned long long)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
}

// One workgroup: block_ofs[0 .. n) becomes its exclusive scan, block_ofs[n] the total.  Thread t owns a contiguous run.
constexpr int kTsdfScanThreads = 1024;
__global__ __launch_bounds__(kTsdfScanThreads) void k_tsdf_scan(unsigned long long* ofs, unsigned n)
{
    __shared__ unsigned long long s[kTsdfScanThreads];
    const unsigned run = (n + kTsdfScanThreads - 1) / kTsdfScanThreads;
    const unsigned lo = min(threadIdx.x * run, n), hi = min(lo + run, n);
    unsigned long long sum = 0;
    for(unsigned q = lo; q < hi; ++q)
        sum += ofs[q];
    s[threadIdx.x] = sum;
    __syncthreads();
    for(int o = 1; o < kTsdfScanThreads; o <<= 1) // inclusive scan of the run sums
    {
        const unsigned long long add = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long acc = s[threadIdx.x] - sum;
    for(unsigned q = lo; q < hi; ++q)
    {
        const unsigned long long v = ofs[q];
        ofs[q] = acc;
        acc += v;
    }
    if(threadIdx.x == kTsdfScanThreads - 1)
        ofs[n] = s[threadIdx.x];
}

__global__ __launch_bounds__(kTsdfThreads) void k_tsdf_write(const TsdfExtractArgs g)
{
    __shared__ int s[kTsdfThreads];
    const TsdfCell c = tsdf_cell(g, (size_t)blockIdx.x * kTsdfThreads + threadIdx.x);
    const int mine = __popc(c.cross);
    s[threadIdx.x] = mine;
    __syncthreads();
    for(int o = 1; o < kTsdfThreads; o <<= 1)
    {
        const int add = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    if(!mine)
        return;
    unsigned long long row = g.block_ofs[blockIdx.x] + (unsigned long long)(s[threadIdx.x] - mine);
    const double fa = (double)c.a.x / (double)c.a.y;
    double fb[3] = {0, 0, 0};
    for(int e = 0; e < 3; ++e)
        if(c.ok[e])
            fb[e] = (double)c.b[e].x / (double)c.b[e].y;
    float nrm[3] = {0.f, 0.f, 0.f};
    if(c.ok[0] && c.ok[1] && c.ok[2])
    {
        const double gx = fb[0] - fa, gy = fb[1] - fa, gz = fb[2] - fa;
        const double len = sqrt((gx * gx + gy * gy) + gz * gz);
        if(len > 0.0)
            nrm[0] = (float)(gx / len), nrm[1] = (float)(gy / len), nrm[2] = (float)(gz / len);
    }
    const double ctr[3] = {g.ox + ((double)c.i + 0.5) * g.voxel, g.oy + ((double)c.j + 0.5) * g.voxel, g.oz + ((double)c.k + 0.5) * g.voxel};
    for(int e = 0; e < 3; ++e)
    {
        if(!(c.cross >> e & 1))
            continue;
        double p[3] = {ctr[0], ctr[1], ctr[2]};
        p[e] = p[e] + (fa / (fa - fb[e])) * g.voxel;
        for(int q = 0; q < 3; ++q)
        {
            g.xyz[row * 3 + q] = (float)p[q];
            g.normal[row * 3 + q] = nrm[q];
        }
        ++row;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static bool finite_all(const double* v, int n)
{
    for(int i = 0; i < n; ++i)
        if(!std::isfinite(v[i]))
            return false;
    return true;
}

// Applies the entries to the volume, MSLAM_HIP_TSDF_CHUNK per sweep: one upload, ceil(n / CHUNK) launches, then the stream is
// drained (the table is read from `entries`, and a removed frame's image is freed by the caller).
static int tsdf_apply(mslam_hip_ctx* c, TsdfState* s, const std::vector<TsdfEntry>& entries, const char* who)
{
    if(entries.empty())
        return MSLAM_HIP_OK;
    hipError_t e = grow(s->d_entries, entries.size(), c->stream);
    if(e == hipSuccess)
        e = hipMemcpyAsync(s->d_entries, entries.data(), entries.size() * sizeof(TsdfEntry), hipMemcpyHostToDevice, c->stream);
    const mslam_hip_tsdf_params& p = s->p;
    TsdfSweepArgs a{};
    a.vol = s->vol;
    a.nx = p.nx, a.ny = p.ny, a.nz = p.nz;
    a.tiles_x = (unsigned)((p.nx + kTsdfTx - 1) / kTsdfTx), a.tiles_y = (unsigned)((p.ny + kTsdfTy - 1) / kTsdfTy);
    const unsigned long long tiles = (unsigned long long)a.tiles_x * a.tiles_y * (unsigned)((p.nz + kTsdfTz - 1) / kTsdfTz);
    a.n_tiles = (unsigned)tiles; // <= 2^30 voxels: below 2^29 tiles even for a volume one voxel thick
    a.voxel = p.voxel, a.ox = p.origin[0], a.oy = p.origin[1], a.oz = p.origin[2], a.trunc = p.trunc, a.max_depth = p.max_depth;
    a.width = p.width, a.height = p.height, a.factor = p.factor;
    a.fx = p.fx, a.fy = p.fy, a.cx = p.cx, a.cy = p.cy;
    const unsigned grid = (unsigned)std::min<unsigned long long>(tiles, kTsdfMaxBlocks);
    for(size_t first = 0; e == hipSuccess && first < entries.size(); first += MSLAM_HIP_TSDF_CHUNK)
    {
        a.e = s->d_entries.get() + first;
        a.n = (int)std::min<size_t>(MSLAM_HIP_TSDF_CHUNK, entries.size() - first);
        StageScope t(c, "tsdf_sweep");
        hipLaunchKernelGGL(k_tsdf_sweep, dim3(grid), dim3(kTsdfThreads), 0, c->stream, a);
        e = hipGetLastError();
    }
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": " + hipGetErrorString(e));
    return MSLAM_HIP_OK;
}

static TsdfEntry tsdf_entry(const TsdfFrame& f, const double* pose, int sign)
{
    TsdfEntry en{};
    std::memcpy(en.R, pose, 9 * sizeof(double));
    std::memcpy(en.t, pose + 9, 3 * sizeof(double));
    en.depth = f.depth;
    en.sign = sign;
    return en;
}

static int tsdf_add(mslam_hip_ctx* c, int frame_id, const uint16_t* depth, const double* R, const double* t, bool from_device,
                    const char* who)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": no volume (mslam_hip_tsdf_create)");
    if(!depth || !R || !t)
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": NULL depth, R or t");
    if(!finite_all(R, 9) || !finite_all(t, 3))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": a non-finite pose entry");
    if(s->frames.count(frame_id))
        return fail(c, MSLAM_HIP_E_INVALID, std::string(who) + ": the frame id exists");
    if((int)s->frames.size() >= s->p.max_frames)
        return fail(c, MSLAM_HIP_E_CAPACITY, std::string(who) + ": max_frames frames are retained");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": hipSetDevice");
    TsdfFrame f;
    const size_t px = (size_t)s->p.width * (size_t)s->p.height;
    hipError_t e = f.depth.alloc(px);
    if(e == hipSuccess)
        e = hipMemcpyAsync(f.depth, depth, px * sizeof(uint16_t), from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string(who) + ": " + hipGetErrorString(e));
    std::memcpy(f.pose, R, 9 * sizeof(double));
    std::memcpy(f.pose + 9, t, 3 * sizeof(double));
    const int rc = tsdf_apply(c, s, {tsdf_entry(f, f.pose, +1)}, who);
    if(rc)
        return rc;
    s->frames.emplace(frame_id, std::move(f));
    return MSLAM_HIP_OK;
}

} // namespace mslam

using namespace mslam;

extern "C" int mslam_hip_tsdf_create(mslam_hip_ctx* c, const mslam_hip_tsdf_params* p)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(!p)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_create: NULL parameters");
    if(p->nx < 1 || p->ny < 1 || p->nz < 1 || (long long)p->nx * p->ny > MSLAM_HIP_TSDF_MAX_VOXELS ||
       (long long)p->nx * p->ny * p->nz > MSLAM_HIP_TSDF_MAX_VOXELS)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_create: nx, ny, nz must be >= 1 with at most 2^30 voxels");
    if(p->max_frames < 1 || p->max_frames > MSLAM_HIP_TSDF_MAX_FRAMES)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_create: max_frames must be 1..32768");
    if(p->width < 1 || p->height < 1 || (long long)p->width * p->height > (1 << 30))
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_create: bad image size");
    if(!std::isfinite(p->voxel) || !(p->voxel > 0) || !std::isfinite(p->trunc) || !(p->trunc > 0) || !(p->max_depth > 0) ||
       !finite_all(p->origin, 3))
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_create: voxel and trunc must be finite and > 0, max_depth > 0, the origin finite");
    if(!(p->fx != 0) || !(p->fy != 0) || std::isnan(p->fx) || std::isnan(p->fy))
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_create: a focal length of zero or NaN");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "tsdf_create: hipSetDevice");
    std::unique_ptr<TsdfState> s(new TsdfState);
    s->p = *p;
    s->p.reserved = 0;
    s->n_voxels = (size_t)p->nx * (size_t)p->ny * (size_t)p->nz;
    hipError_t e = hipStreamSynchronize(c->stream); // nothing reads the volume this one replaces
    if(e == hipSuccess)
        e = s->vol.alloc(s->n_voxels);
    if(e == hipSuccess)
        e = hipMemsetAsync(s->vol, 0, s->n_voxels * sizeof(int2), c->stream);
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string("tsdf_create: ") + hipGetErrorString(e));
    tsdf_destroy(c->tsdf);
    c->tsdf = s.release();
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_destroy(mslam_hip_ctx* c)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(c->tsdf)
    {
        (void)hipSetDevice(c->p.device);
        (void)hipStreamSynchronize(c->stream);
        tsdf_destroy(c->tsdf);
        c->tsdf = nullptr;
    }
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_info(mslam_hip_ctx* c, mslam_hip_tsdf_params* out, int* n_frames)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(!c->tsdf)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_info: no volume (mslam_hip_tsdf_create)");
    if(out)
        *out = c->tsdf->p;
    if(n_frames)
        *n_frames = (int)c->tsdf->frames.size();
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_add_frame(mslam_hip_ctx* c, int frame_id, const uint16_t* depth, const double* R, const double* t)
{
    return tsdf_add(c, frame_id, depth, R, t, false, "tsdf_add_frame");
}

extern "C" int mslam_hip_tsdf_add_frame_dev(mslam_hip_ctx* c, int frame_id, const uint16_t* d_depth, const double* R, const double* t)
{
    return tsdf_add(c, frame_id, d_depth, R, t, true, "tsdf_add_frame_dev");
}

extern "C" int mslam_hip_tsdf_get_frame(mslam_hip_ctx* c, int frame_id, double* R, double* t)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    if(!c->tsdf)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_get_frame: no volume (mslam_hip_tsdf_create)");
    if(!R || !t)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_get_frame: NULL R or t");
    const auto it = c->tsdf->frames.find(frame_id);
    if(it == c->tsdf->frames.end())
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_get_frame: unknown frame id");
    std::memcpy(R, it->second.pose, 9 * sizeof(double));
    std::memcpy(t, it->second.pose + 9, 3 * sizeof(double));
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_update_poses(mslam_hip_ctx* c, const int32_t* frame_ids, const double* R, const double* t, int n,
                                           int* n_moved)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_update_poses: no volume (mslam_hip_tsdf_create)");
    if(n < 0 || (n > 0 && (!frame_ids || !R || !t)))
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_update_poses: n < 0 or a NULL list");
    std::set<int> seen;
    for(int q = 0; q < n; ++q)
    {
        if(!s->frames.count(frame_ids[q]))
            return fail(c, MSLAM_HIP_E_INVALID, "tsdf_update_poses: unknown frame id");
        if(!seen.insert(frame_ids[q]).second)
            return fail(c, MSLAM_HIP_E_INVALID, "tsdf_update_poses: a frame id is listed twice");
        if(!finite_all(R + 9 * (size_t)q, 9) || !finite_all(t + 3 * (size_t)q, 3))
            return fail(c, MSLAM_HIP_E_INVALID, "tsdf_update_poses: a non-finite pose entry");
    }
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "tsdf_update_poses: hipSetDevice");
    // a frame's -1 entry comes before its +1 entry: no partial sum leaves the range |S| < 2^30 + 2^15 promises
    std::vector<TsdfEntry> entries;
    std::vector<int> moved;
    for(int q = 0; q < n; ++q)
    {
        const TsdfFrame& f = s->frames.find(frame_ids[q])->second;
        double pose[12];
        std::memcpy(pose, R + 9 * (size_t)q, 9 * sizeof(double));
        std::memcpy(pose + 9, t + 3 * (size_t)q, 3 * sizeof(double));
        if(std::memcmp(pose, f.pose, sizeof(pose)) == 0)
            continue;
        entries.push_back(tsdf_entry(f, f.pose, -1));
        entries.push_back(tsdf_entry(f, pose, +1));
        moved.push_back(q);
    }
    const int rc = tsdf_apply(c, s, entries, "tsdf_update_poses");
    if(rc)
        return rc;
    for(int q : moved)
    {
        TsdfFrame& f = s->frames.find(frame_ids[q])->second;
        std::memcpy(f.pose, R + 9 * (size_t)q, 9 * sizeof(double));
        std::memcpy(f.pose + 9, t + 3 * (size_t)q, 3 * sizeof(double));
    }
    if(n_moved)
        *n_moved = (int)moved.size();
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_remove_frame(mslam_hip_ctx* c, int frame_id)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_remove_frame: no volume (mslam_hip_tsdf_create)");
    const auto it = s->frames.find(frame_id);
    if(it == s->frames.end())
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_remove_frame: unknown frame id");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "tsdf_remove_frame: hipSetDevice");
    const int rc = tsdf_apply(c, s, {tsdf_entry(it->second, it->second.pose, -1)}, "tsdf_remove_frame");
    if(rc)
        return rc;
    s->frames.erase(it); // the stream has drained: nothing reads the image any more
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_read(mslam_hip_ctx* c, int32_t* S, int32_t* W)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_read: no volume (mslam_hip_tsdf_create)");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "tsdf_read: hipSetDevice");
    const size_t slab = (size_t)1 << 22; // voxels per copy
    std::vector<int2> host(std::min(slab, s->n_voxels));
    for(size_t first = 0; first < s->n_voxels; first += slab)
    {
        const size_t m = std::min(slab, s->n_voxels - first);
        hipError_t e = hipMemcpyAsync(host.data(), s->vol.get() + first, m * sizeof(int2), hipMemcpyDeviceToHost, c->stream);
        if(e == hipSuccess)
            e = hipStreamSynchronize(c->stream);
        if(e != hipSuccess)
            return fail(c, MSLAM_HIP_E_RUNTIME, std::string("tsdf_read: ") + hipGetErrorString(e));
        for(size_t q = 0; q < m; ++q)
        {
            if(S)
                S[first + q] = host[q].x;
            if(W)
                W[first + q] = host[q].y;
        }
    }
    return MSLAM_HIP_OK;
}

extern "C" int mslam_hip_tsdf_extract(mslam_hip_ctx* c, int min_weight, float* xyz, float* normal, int capacity, int* n)
{
    if(!c)
        return MSLAM_HIP_E_INVALID;
    TsdfState* s = c->tsdf;
    if(!s)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_extract: no volume (mslam_hip_tsdf_create)");
    if(!n || capacity < 0 || (capacity > 0 && !xyz) || min_weight < 1)
        return fail(c, MSLAM_HIP_E_INVALID, "tsdf_extract: NULL n, NULL xyz with a capacity, capacity < 0 or min_weight < 1");
    if(hipSetDevice(c->p.device) != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, "tsdf_extract: hipSetDevice");
    TsdfExtractArgs g{};
    g.vol = s->vol;
    g.nx = s->p.nx, g.ny = s->p.ny, g.nz = s->p.nz;
    g.n_voxels = s->n_voxels;
    g.min_weight = min_weight;
    g.voxel = s->p.voxel, g.ox = s->p.origin[0], g.oy = s->p.origin[1], g.oz = s->p.origin[2];
    g.n_blocks = (unsigned)((s->n_voxels + kTsdfThreads - 1) / kTsdfThreads);
    hipError_t e = grow(s->d_block_ofs, (size_t)g.n_blocks + 1, c->stream);
    g.block_ofs = s->d_block_ofs;
    unsigned long long total = 0;
    if(e == hipSuccess)
    {
        StageScope t(c, "tsdf_count");
        hipLaunchKernelGGL(k_tsdf_count, dim3(g.n_blocks), dim3(kTsdfThreads), 0, c->stream, g);
        hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(kTsdfScanThreads), 0, c->stream, g.block_ofs, g.n_blocks);
        e = hipGetLastError();
    }
    if(e == hipSuccess)
        e = hipMemcpyAsync(&total, g.block_ofs + g.n_blocks, sizeof(total), hipMemcpyDeviceToHost, c->stream);
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string("tsdf_extract: ") + hipGetErrorString(e));
    *n = (int)std::min<unsigned long long>(total, 0x7fffffffull);
    if(total > (unsigned long long)capacity)
        return fail(c, MSLAM_HIP_E_CAPACITY, "tsdf_extract: more surface points than capacity (*n rows are needed)");
    if(total == 0)
        return MSLAM_HIP_OK;
    const size_t rows = (size_t)total * 3;
    e = grow(s->d_xyz, rows, c->stream);
    if(e == hipSuccess)
        e = grow(s->d_normal, rows, c->stream);
    g.xyz = s->d_xyz, g.normal = s->d_normal;
    if(e == hipSuccess)
    {
        StageScope t(c, "tsdf_write");
        hipLaunchKernelGGL(k_tsdf_write, dim3(g.n_blocks), dim3(kTsdfThreads), 0, c->stream, g);
        e = hipGetLastError();
    }
    if(e == hipSuccess)
        e = hipMemcpyAsync(xyz, s->d_xyz, rows * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if(e == hipSuccess && normal)
        e = hipMemcpyAsync(normal, s->d_normal, rows * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if(e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    if(e != hipSuccess)
        return fail(c, MSLAM_HIP_E_RUNTIME, std::string("tsdf_extract: ") + hipGetErrorString(e));
    return MSLAM_HIP_OK;
}
