// icp.hpp — the scratch of frame-to-model alignment (k_icp.hip, mslam_hip_icp_* and mslam_hip_tsdf_icp*): one per context,
// grown on demand, needs no volume.
#pragma once
#include "devmem.hpp"
#include "../../include/mslam_hip.h"

namespace mslam
{
// What the kernels of one solve share.  The frame kernel writes the start state, every finish kernel the rest; a launch reads
// `done` and `level` first and returns when the solve or its level has ended.
struct IcpCtrl
{
    double Q[9], s[3];  // the state: camera -> world
    double sums[32];    // the last linearisation: A21, g6, sum r r, the count (exact in f64)
    double pivots[6];
    double R[9], t[3];  // world -> camera, written when the solve ends
    int32_t done, status, level, n_lin, count, last_level, pad[2];
    double cost;
};

struct IcpState
{
    DevBuf<uint16_t> d_depth;      // the frame of a call with a host image
    DevBuf<float> d_mxyz, d_mnrm;  // the model of a call with host images
    DevBuf<double> d_frame;        // six planes [height][width]: V0 V1 V2 n0 n1 n2 (f64: an f32 copy would change bits)
    DevBuf<uint8_t> d_has;         // [height][width]: the pixel has a frame normal
    DevBuf<double> d_part;         // [chunks of the finest level][32]: one row of partial sums per workgroup
    DevBuf<uint8_t> d_ctrl;        // IcpCtrl, then MSLAM_HIP_ICP_MAX_ITERATIONS record rows
};
} // namespace mslam
