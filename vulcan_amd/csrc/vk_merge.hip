// vk_merge.hip — fuse one voxel-hashed volume into another, for gfx950
// (ref: src/volume.cu:304-368 HandleAllocationRequests allocates the blocks the destination lacks, through the existing
// handle pass; src/depth_integrator.cu:55-59 and src/color_integrator.cu:109-118 are the running averages the fusion
// continues. Upstream's Volume is a process-wide singleton, src/volume.cu:17-21: there is no counterpart. The definition
// is in include/vk.h at vk_volume_merge; tests/merge_reference.py states it on the CPU and the device is held to it bit
// for bit).
//
// Shape: everything is enqueued on the caller's stream and nothing is read back. Every decision compares stored values,
// every count is an integer sum and a bucket's contest is won by the largest key, so no result depends on the order in
// which workgroups or atomics arrive.
//   init      per source entry: state, no destination slot known; the words that steer the rounds
//   mark      one thread per source bucket walks its chain and marks the entries that hold a block
//   classify  (SKIP_UNOBSERVED only) one wave per marked entry streams the block and drops it when no voxel has a weight:
//             the one extra read of the source pool
//   rounds    max_rounds times: request pass, the existing handle pass (vk_volume_handle_allocation_requests), round end.
//             A round that finds the rounds over posts nothing, and its handle pass then changes nothing.
//   resolve   the request pass once more, without posting: the slots of the blocks the last round allocated
//   finish    the six counts, VK_CTR_VISIBLE and VK_CTR_BANDED
//   fuse      one wave per source block with a destination slot: the only pass over the two voxel pools
// All passes but mark are vk_merge_passes.hpp's, which vk_volume_merge_packed (vk_pack.hip) runs over a pack's blocks.
#include "vk_merge_passes.hpp"

using namespace vk;

namespace
{

// a source block is an entry of the source volume's table (vk_merge_passes.hpp)
struct VolumeSource
{
  static constexpr bool kListed = false;
  vk_volume v;
  int total;                    // main + excess entries = pool slots
  __host__ __device__ __forceinline__ int count() const { return total; }
  __device__ __forceinline__ Entry origin(int index) const { return load_entry(v.hash_entries, (uint32_t)index); }
  __device__ __forceinline__ const uint4* block(int index) const { return pool_block(v.voxels, v.hash_entries[index].data); }
};

typedef MergeParams<VolumeSource> VolumeMerge;

// one thread per source bucket: its source blocks (mark_chain)
__global__ __launch_bounds__(256) void merge_mark_kernel(VolumeMerge P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  const int blocks = mark_chain(P.src.v, P.src.total, bucket, [&](int index) { P.state[index] = kConsidered; });
  if (!(P.flags & VK_MERGE_SKIP_UNOBSERVED)) wave_add(&P.ctl[cConsidered], blocks);   // (classify counts otherwise)
}

}  // namespace

extern "C" {

size_t vk_volume_merge_workspace_bytes(int32_t src_main, int32_t src_excess)
{
  if (src_main <= 0 || src_excess < 0) return 0;
  const size_t total = (size_t)src_main + (size_t)src_excess;
  if (total > (size_t)INT32_MAX) return 0;
  return merge_workspace_bytes(total);
}

int vk_volume_merge(const vk_volume* dst, const vk_volume* src, const vk_merge_params* p, int32_t* counts_dev, void* workspace,
    void* stream)
{
  VK_REQUIRE(dst && src && p && counts_dev && workspace);
  VK_REQUIRE(merge_ok(dst, src, *p));
  hipStream_t s = vk_s(stream);
  VolumeMerge P;
  P.dst = *dst;
  P.src.v = *src;
  P.src.total = src->main_block_count + src->excess_block_count;
  P.flags = p->flags;
  P.cap_distance = p->max_distance_weight;
  P.cap_color = p->max_color_weight;
  P.dst_total = dst->main_block_count + dst->excess_block_count;
  merge_carve_workspace(P, workspace);
  P.counts = counts_dev;

  const int bucket_groups = (src->main_block_count + 255) / 256, entry_groups = (P.src.total + 255) / 256;
  VK_CHECK(hipMemsetAsync(P.ctl, 0, cWords * sizeof(int32_t), s));
  hipLaunchKernelGGL(merge_init_kernel<VolumeSource>, dim3(entry_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  if (!(p->flags & VK_MERGE_CONTINUE))
  {
    hipLaunchKernelGGL(merge_mark_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
    VK_LAUNCH_CHECK();
  }
  return merge_enqueue_passes(dst, p, P, stream);
}

}  // extern "C"
