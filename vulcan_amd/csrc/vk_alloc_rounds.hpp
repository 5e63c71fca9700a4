// vk_alloc_rounds.hpp — the allocation rounds of the operations that give a volume new blocks (vk_merge.hip,
// vk_merge_pose.hip, vk_integrate_rays.hip): max_rounds times a request pass of the caller's own, the existing handle pass
// (vk_volume_handle_allocation_requests, ref: src/volume.cu:304-368) and the round end. A round that finds the rounds over
// posts nothing, and its handle pass then changes nothing. Everything is enqueued and nothing is read back.
#pragma once

#include "vk_block_walk.hpp"

namespace vk
{

// the words that steer the rounds: the first of a caller's cWords control words, its own follow from cRoundWords
enum { cStop = 0, cPosted, cRounds, cSavedRequests, cDroppedBefore, cRoundWords };

// the start of a call (one thread; the control words are zero): what the rounds must leave in the two counters
__device__ __forceinline__ void rounds_begin(int32_t* ctl, const int32_t* counters)
{
  ctl[cSavedRequests] = counters[VK_CTR_REQUESTS];
  ctl[cDroppedBefore] = counters[VK_CTR_DROPPED];
}

// The absent block (bx, by, bz) asks for a slot the way SetView's request pass does (post_request, the largest 64-bit key
// wins the bucket; a MAIN request marks the bucket visible, volume.cu:193-200). `main_entry`: its bucket's, from find_block.
// The caller counts the request into ctl[cPosted].
__device__ __forceinline__ void request_block(const vk_volume& v, int bx, int by, int bz, const Entry& main_entry)
{
  const Retry none = {};                            // nothing is recorded for later rounds: every round looks again
  const uint32_t bucket = block_hash(bx, by, bz, (uint32_t)v.main_block_count);
  const int type = main_entry.data == -1 ? VK_ALLOC_MAIN : VK_ALLOC_EXCESS;
  if (type == VK_ALLOC_MAIN && v.block_visibility[bucket] != VK_VISIBILITY_TRUE) v.block_visibility[bucket] = VK_VISIBILITY_TRUE;
  post_request(v, bucket, type, bx, by, bz, none, bucket);
}

// One thread, behind a round's handle pass. A handle pass that found no request has only written VK_CTR_REQUESTS = 0:
// put back what the last round that did something left there.
static __global__ void round_end_kernel(int32_t* ctl, int32_t* counters)
{
  if (ctl[cStop] || ctl[cPosted] == 0)
  {
    ctl[cStop] = 1;
    counters[VK_CTR_REQUESTS] = ctl[cSavedRequests];
    return;
  }
  ctl[cRounds] += 1;
  ctl[cPosted] = 0;
  ctl[cSavedRequests] = counters[VK_CTR_REQUESTS];
  if (counters[VK_CTR_DROPPED] != ctl[cDroppedBefore]) ctl[cStop] = 1;      // divergence 14: a round that drops ends the rounds
}

// the end of a call (one thread): the operation moved blocks under the lists of the last SetView
__device__ __forceinline__ void lists_stale(int32_t* counters)
{
  counters[VK_CTR_VISIBLE] = 0;
  counters[VK_CTR_BANDED] = -1;                   // the banded lists list nothing any more
}

// The host's loop. request_pass() launches the caller's request kernel, which returns at once when ctl[cStop] is set and
// adds what it posts to ctl[cPosted].
template <class RequestPass>
int run_rounds(const vk_volume* v, int max_rounds, int32_t* ctl, void* stream, RequestPass&& request_pass)
{
  for (int round = 0; round < max_rounds; ++round)
  {
    request_pass();
    VK_LAUNCH_CHECK();
    const int code = vk_volume_handle_allocation_requests(v, stream);
    if (code != VK_OK) return code;
    hipLaunchKernelGGL(round_end_kernel, dim3(1), dim3(1), 0, vk_s(stream), ctl, v->counters);
    VK_LAUNCH_CHECK();
  }
  return VK_OK;
}

// what vk_volume_merge and vk_volume_merge_posed ask of their arguments
inline bool merge_params_ok(const vk_merge_params& m)
{
  return (m.flags & ~(VK_MERGE_SKIP_UNOBSERVED | VK_MERGE_CONTINUE)) == 0 && m.max_rounds >= 1 &&
         m.max_distance_weight >= 1.0f && m.max_distance_weight <= 32767.0f &&        // (false for a NaN)
         m.max_color_weight >= 1.0f && m.max_color_weight <= 32767.0f;
}

inline bool merge_ok(const vk_volume* dst, const vk_volume* src, const vk_merge_params& m)
{
  return volumes_match(dst, src) && dst->voxels != src->voxels && merge_params_ok(m);
}

}  // namespace vk
