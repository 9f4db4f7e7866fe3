// tsdf.hpp — the dense map behind mslam_hip_tsdf_* (k_tsdf.hip, k_tsdf_raycast.hip): the volume, the retained frames and the
// scratch of the extraction and of the ray-cast.  The invariant: `vol` equals the integration of `frames` at their stored poses
// into a zeroed volume.
#pragma once
#include "devmem.hpp"
#include "../../include/mslam_hip.h"
#include <map>

namespace mslam
{
// One (frame, sign) entry of a batched sweep, as the kernel reads it (wave-uniform, hence scalar loads).
struct TsdfEntry
{
    double R[9], t[3];     // world -> camera
    const uint16_t* depth; // [height][width] on the device
    int32_t sign, pad;     // +1 integrate, -1 de-integrate
};

struct TsdfFrame
{
    DevBuf<uint16_t> depth;
    double pose[12]; // R (9, row-major), t (3): the pose the frame is integrated at
};

struct TsdfState
{
    mslam_hip_tsdf_params p{};
    size_t n_voxels = 0;
    DevBuf<int2> vol;                // [nz][ny][nx] of (S, W): one 8-byte access per voxel and sweep
    std::map<int, TsdfFrame> frames; // by frame id
    DevBuf<TsdfEntry> d_entries;     // the entries of one call, grown on demand
    // extraction: crossings per workgroup and their exclusive scan (the last element is the total), the rows
    DevBuf<unsigned long long> d_block_ofs;
    DevBuf<float> d_xyz, d_normal;
    // ray-cast (k_tsdf_raycast.hip): hits per workgroup, and the depth image of a call with host pointers (its point and
    // normal images use d_xyz and d_normal)
    DevBuf<unsigned> d_ray_hits;
    DevBuf<float> d_ray_depth;
};
} // namespace mslam
