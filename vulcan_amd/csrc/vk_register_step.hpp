// vk_register_step.hpp — the solve of one registration step, shared by vk_register.hip (volume against volume) and
// vk_register_rays.hip (a sweep of range rays against a volume): both end a step the same way, word for word (include/vk.h at
// vk_volume_register: the step, the state, the end of the loop).
#pragma once

#include "vk_gauss_newton.hpp"

namespace vk
{

// One wave: the colour trackers' step on the pose itself. M = Tinc(update) * m, pose <- rigid_from(M). counts[2] is the
// step's number of residuals. (static: each file that launches it holds its own copy of the kernel.)
static __global__ __launch_bounds__(64) void register_solve_kernel(const float* __restrict__ system, const int32_t* __restrict__ counts,
    vk_transform* pose, int32_t* state, float* update_out)
{
  if (state[1]) return;
  if (counts[2] == 0)
  {
    if (threadIdx.x == 0)
    {
      state[0] += 1;
      state[1] = VK_REGISTER_NO_OVERLAP;
      if (update_out)
        for (int i = 0; i < 6; ++i) update_out[i] = 0.0f;
    }
    return;
  }
  float update[6], M[16], out_m[16], out_i[16];
  staged_pose_step<6, -1>(system, system + 36, pose->m, M, update);
  if (threadIdx.x != 0) return;
  bool moves = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) moves = moves || update[i] != 0.0f;
  if (moves)                                      // a zero update (no gradient, or a rank-deficient system) leaves the bytes alone
  {
    rigid_from(M, out_m, out_i);
#pragma unroll
    for (int i = 0; i < 16; ++i) { pose->m[i] = out_m[i]; pose->inv[i] = out_i[i]; }
  }
  finish_step<6>(update, state, update_out);
}

}  // namespace vk
