// fuse_launch.hip -- host side of the fused field query: the planner's choice (EvalParams, d3f_plan.h) -> the family's launcher.
#include <hip/hip_runtime.h>

#include "d3f_internal.h"

namespace d3f {

hipError_t launch_fused_eval(const EvalParams &P, FamilyId family, int mode, const Launch &L)
{
    if (P.n == 0 && !L.describe) return hipSuccess;
    switch (family) {
    case kFamDistOnly: return launch_dist(P, mode, L);
    case kFamWindow: return launch_window(P, L);
    case kFamRuns: return launch_runs(P, L);
    case kFamSliced: return launch_sliced(P, L);
    case kFamRows: return launch_rows(P, L);
    case kFamDirect: return launch_direct(P, L);
    }
    return hipErrorInvalidValue;
}

}  // namespace d3f
