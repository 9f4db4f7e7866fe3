// Stand-alone host check of StageScope (csrc/context.hpp) under AddressSanitizer: scopes nested the way the bundle
// adjustment nests them (solver_schur / solver_factor / solver_subst inside ba_iterations) on a context whose timer vector
// is empty, so that the inner scopes' push_back moves the vector while the outer scope is open.  The HIP event calls are
// replaced by host stubs (no GPU is touched); every event handle is a heap block of its own, so a record on a stale or
// freed handle is an ASan report.  Build and run (no GPU needed):
//   g++ -std=c++17 -g -fsanitize=address -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Imodular-slam_amd/csrc -Iinclude
//       tools/experiments/stage_scope_nesting.cpp -o tools/experiments/stage_scope_nesting_probe && ./tools/experiments/stage_scope_nesting_probe
// With StageScope holding a pointer into the vector (before the fix) ASan reports heap-use-after-free in ~StageScope; with
// the index it prints "ok".
#include "context.hpp"

#include <cstdio>
#include <cstdlib>

static int g_records = 0;
extern "C" hipError_t hipEventCreate(hipEvent_t* e)
{
    *e = reinterpret_cast<hipEvent_t>(new int(0));
    return hipSuccess;
}
extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    *reinterpret_cast<int*>(e) += 1; // touches the handle: a garbage handle faults here
    ++g_records;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void*) { return hipSuccess; }
extern "C" hipError_t hipHostFree(void*) { return hipSuccess; }

int main()
{
    mslam_hip_ctx* c = new mslam_hip_ctx();
    c->inplace_timing = true;
    int scopes = 0;
    for(int solve = 0; solve < 3; ++solve) // the first solve grows the vector, the later ones reuse entries after a read
    {
        for(int batch = 0; batch < 5; ++batch)
        {
            mslam::StageScope outer(c, "ba_iterations");
            ++scopes;
            for(int it = 0; it < 4; ++it)
            {
                {
                    mslam::StageScope a(c, "solver_schur");
                    ++scopes;
                }
                {
                    mslam::StageScope b(c, "solver_factor");
                    ++scopes;
                }
                mslam::StageScope d(c, "solver_subst");
                ++scopes;
            }
        }
        if(solve == 1)
            c->timers_used = 0; // what mslam_hip_get_stage_times does after reading
    }
    // every scope recorded its own start and stop exactly once
    for(size_t i = 0; i < c->timers.size(); ++i)
    {
        const int s = *reinterpret_cast<int*>(c->timers[i].start), e = *reinterpret_cast<int*>(c->timers[i].stop);
        if(s != e || s < 1)
        {
            std::printf("timer %zu: %d starts, %d stops\n", i, s, e);
            return 1;
        }
    }
    if(g_records != 2 * scopes)
    {
        std::printf("%d records for %d scopes\n", g_records, scopes);
        return 1;
    }
    std::printf("ok: %d scopes, %zu timers\n", scopes, c->timers.size());
    return 0;
}
