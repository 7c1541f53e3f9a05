// gte_hot_body.h — what gte_hot.hip and gte_hot_nt.hip compile: the launcher and the occupancy query
// of the headline instantiation.  The including unit defines GTE_HOT_NT (the observation store
// policy, store_out<NT>), GTE_HOT_NAME(x) (the suffix of the two functions' names) and GTE_HOT_ONLY
// (gte_device.h, hot_tu_covers) first.
#include "gte_step.h"

namespace gte {

hipError_t GTE_HOT_NAME(launch_step_hot)(const Params& p, int blocks, int threads, size_t smem,
                                         hipStream_t stream) {
  if (!hot_tu_covers(p)) return hipErrorInvalidValue;  // features compiled out of this TU (gte_device.h)
  const uint32_t V = (uint32_t)(p.W * p.Fobs);
  const uint64_t vm = magic40(V / 4), fm = magic40((uint32_t)p.Fobs / 4),
                 wm = magic40((uint32_t)(p.W * (p.nd ? p.nd : 1)));
  hipLaunchKernelGGL((gte_kernel<MODE_STEP, 4, GTE_HOT_NT, true, STAGE_RAW>), dim3(blocks),
                     dim3(threads), smem, stream, p, vm, fm, wm);
  return hipGetLastError();
}

// Workgroups of this kernel one CU holds at once (registers, LDS): the launch geometry sizes
// the workgroups so that all of them are resident together (gte_plan.h, step_geometry).
int GTE_HOT_NAME(hot_blocks_per_cu)(size_t smem) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &n, gte_kernel<MODE_STEP, 4, GTE_HOT_NT, true, STAGE_RAW>, 64 * GTE_WAVES, smem) != hipSuccess)
    return 0;
  return n;
}

}  // namespace gte
