// vk_pack.hip — a volume's blocks as one compact object in a defined order, and the merge that takes such an object in
// a source volume's place, for gfx950
// (ref: src/volume.cu:17-21 upstream's Volume is a process-wide singleton that never leaves its buffers: there is no
// counterpart; src/volume.cu:183-190 is the chain walk that names the blocks. The definitions are in include/vk.h at
// vk_volume_pack and vk_volume_merge_packed; tests/pack_reference.py states them on the CPU and the device is held to
// them byte for byte).
//
// vk_volume_pack: everything is enqueued on the caller's stream and nothing is read back. A block's position in the pack
// comes from an ordered scan over the table, so no atomic decides one.
//   clear     one memset: the control words and the per-entry flags
//   mark      one thread per main bucket walks its chain (mark_chain), applies the box to an entry's origin and flags the
//             entries whose block is selected so far
//   classify  (SKIP_UNOBSERVED only) one wave per flagged entry streams the block and clears the flag when no voxel has
//             a weight (merge's test, wave_block_observed)
//   scan      vk_compact_offsets over the flags: stable, so "ascending entry index" holds by construction
//   list      one thread per entry: entry index of packed block k, for k below the capacity; thread 0 writes the counts
//   gather    one wave per packed block, four per workgroup: ten 16-byte loads, then ten 16-byte stores per lane; lane 0
//             writes the origin. The hot path, and a pure copy.
// vk_volume_merge_packed: the passes of vk_merge_passes.hpp over PackSource — block k's origin and voxels come from the
// pack, everything else is vk_volume_merge's own code.
#include "vk_merge_passes.hpp"

using namespace vk;

namespace
{

// the control words of a pack call
enum { pSource = 0, pSelected, pSkipped, pWords = 16 };

struct PackParams
{
  vk_volume v;
  int total;                    // main + excess entries = pool slots
  int flags;
  int lo[3], hi[3];
  int capacity;
  int16_t* origins;
  vk_voxel* voxels;             // nullptr: count only
  // workspace
  int32_t* ctl;                 // [pWords]
  int32_t* flag;                // [total]  1: the entry's block is selected
  int32_t* offset;              // [total]  its position in the pack, -1 without one
  int32_t* list;                // [total]  entry index of packed block k
  int32_t* counts;              // [4] output
};

// one thread per main bucket: its source blocks (mark_chain), less those the box excludes
__global__ __launch_bounds__(256) void pack_mark_kernel(PackParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  const int blocks = mark_chain(P.v, P.total, bucket, [&](int index) {
    const Entry entry = load_entry(P.v.hash_entries, (uint32_t)index);
    const bool inside = entry.ox >= P.lo[0] && entry.ox <= P.hi[0] && entry.oy >= P.lo[1] && entry.oy <= P.hi[1] &&
                        entry.oz >= P.lo[2] && entry.oz <= P.hi[2];
    if (!(P.flags & VK_PACK_BOX) || inside) P.flag[index] = 1;
  });
  wave_add(&P.ctl[pSource], blocks);
}

// SKIP_UNOBSERVED: one wave per flagged entry
__global__ __launch_bounds__(kWaveThreads) void pack_classify_kernel(PackParams P)
{
  const int index = blockIdx.x * (kWaveThreads / kWave) + (int)(threadIdx.x >> 6);
  if (index >= P.total) return;
  if (P.flag[index] != 1) return;
  const bool observed = wave_block_observed(pool_block(P.v.voxels, P.v.hash_entries[index].data));
  if (lane_id() == 0 && !observed)
  {
    P.flag[index] = 0;
    atomicAdd(&P.ctl[pSkipped], 1);
  }
}

// one thread per entry, behind the scan: which entry packed block k is; the four counts
__global__ __launch_bounds__(256) void pack_list_kernel(PackParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index < P.total && P.voxels)
  {
    const int at = P.offset[index];
    if (at >= 0 && at < P.capacity) P.list[at] = index;
  }
  if (index == 0)
  {
    const int selected = P.ctl[pSelected];
    P.counts[0] = P.ctl[pSource];
    P.counts[1] = selected;
    P.counts[2] = P.voxels ? vmini(selected, P.capacity) : 0;
    P.counts[3] = P.ctl[pSkipped];
  }
}

// One wave per packed block: the block's 640 16-byte vectors, lane l of trip t vector 64 t + l — all ten loads in flight,
// then the ten stores. No LDS, no atomics.
__global__ __launch_bounds__(kWaveThreads) void pack_gather_kernel(PackParams P)
{
  const int k = blockIdx.x * (kWaveThreads / kWave) + (int)(threadIdx.x >> 6);
  if (k >= vmini(P.ctl[pSelected], P.capacity)) return;        // nothing at or behind block `written`
  const int index = P.list[k];
  if (index < 0 || index >= P.total) return;
  const Entry entry = load_entry(P.v.hash_entries, (uint32_t)index);
  if (entry.data < 0 || entry.data >= P.total) return;
  const int lane = lane_id();
  // (a native vector: ten uint4 structs copied whole are kept in scratch, ten of these in registers)
  typedef uint32_t vector16 __attribute__((ext_vector_type(4)));
  const vector16* from = reinterpret_cast<const vector16*>(pool_block(P.v.voxels, entry.data));
  vector16* to = reinterpret_cast<vector16*>(pool_block(P.voxels, k));
  vector16 data[kVectorTrips];
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t) data[t] = from[t * kWave + lane];
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t) to[t * kWave + lane] = data[t];
  if (lane == 0)
    reinterpret_cast<int2*>(P.origins)[k] = make_int2((int)((uint32_t)(uint16_t)entry.ox | ((uint32_t)(uint16_t)entry.oy << 16)),
                                                      (int)(uint32_t)(uint16_t)entry.oz);
}

// a source block is block k of a pack (vk_merge_passes.hpp)
struct PackSource
{
  static constexpr bool kListed = true;
  const int16_t* origins;
  const vk_voxel* voxels;
  int blocks;
  __host__ __device__ __forceinline__ int count() const { return blocks; }
  __device__ __forceinline__ Entry origin(int k) const
  {
    const int2 raw = reinterpret_cast<const int2*>(origins)[k];
    Entry e;
    e.ox = (int16_t)(raw.x & 0xffff);
    e.oy = (int16_t)((uint32_t)raw.x >> 16);
    e.oz = (int16_t)(raw.y & 0xffff);
    e.pad = 0;
    e.data = k;
    e.next = -1;
    return e;
  }
  __device__ __forceinline__ const uint4* block(int k) const { return pool_block(voxels, k); }
};

typedef MergeParams<PackSource> PackMerge;

inline bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }

}  // namespace

extern "C" {

size_t vk_volume_pack_workspace_bytes(int32_t main_block_count, int32_t excess_block_count)
{
  if (main_block_count <= 0 || excess_block_count < 0) return 0;
  const size_t total = (size_t)main_block_count + (size_t)excess_block_count;
  if (total > (size_t)INT32_MAX) return 0;
  return align_up(pWords * 4) + 3 * align_up(total * 4) + align_up(vk_compact_workspace_bytes((int32_t)total));
}

int vk_volume_pack(const vk_volume* v, const vk_pack_rule* rule, const vk_block_pack* pack, int32_t* counts_dev, void* workspace,
    void* stream)
{
  VK_REQUIRE(v && pack && counts_dev && workspace);
  VK_REQUIRE(volume_ok(v));
  VK_REQUIRE(pack->capacity >= 0);
  if (pack->voxels) VK_REQUIRE(pack->origins && aligned(pack->origins, 8) && aligned(pack->voxels, 16));
  PackParams P;
  P.flags = 0;
  for (int a = 0; a < 3; ++a) P.lo[a] = P.hi[a] = 0;
  if (rule)
  {
    VK_REQUIRE((rule->flags & ~(VK_PACK_SKIP_UNOBSERVED | VK_PACK_BOX)) == 0);
    P.flags = rule->flags;
    if (rule->flags & VK_PACK_BOX)
      for (int a = 0; a < 3; ++a)
      {
        VK_REQUIRE(rule->lo[a] <= rule->hi[a]);
        P.lo[a] = rule->lo[a];
        P.hi[a] = rule->hi[a];
      }
  }
  hipStream_t s = vk_s(stream);
  P.v = *v;
  P.total = v->main_block_count + v->excess_block_count;
  P.capacity = pack->capacity;
  P.origins = pack->origins;
  P.voxels = pack->voxels;
  const size_t total = (size_t)P.total;
  char* at = static_cast<char*>(workspace);
  P.ctl = reinterpret_cast<int32_t*>(at);         at += align_up(pWords * 4);
  P.flag = reinterpret_cast<int32_t*>(at);        at += align_up(total * 4);
  P.offset = reinterpret_cast<int32_t*>(at);      at += align_up(total * 4);
  P.list = reinterpret_cast<int32_t*>(at);        at += align_up(total * 4);
  void* scan_workspace = at;
  P.counts = counts_dev;

  const int bucket_groups = (v->main_block_count + 255) / 256, entry_groups = (P.total + 255) / 256;
  const int waves_per_group = kWaveThreads / kWave;
  // (the control words and the flags lie one behind the other)
  VK_CHECK(hipMemsetAsync(P.ctl, 0, align_up(pWords * 4) + total * 4, s));
  hipLaunchKernelGGL(pack_mark_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  if (P.flags & VK_PACK_SKIP_UNOBSERVED)
  {
    hipLaunchKernelGGL(pack_classify_kernel, dim3((P.total + waves_per_group - 1) / waves_per_group), dim3(kWaveThreads), 0, s, P);
    VK_LAUNCH_CHECK();
  }
  const int code = vk_compact_offsets(P.flag, P.total, P.offset, &P.ctl[pSelected], scan_workspace, stream);
  if (code != VK_OK) return code;
  hipLaunchKernelGGL(pack_list_kernel, dim3(entry_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  const int slots = P.capacity < P.total ? P.capacity : P.total;      // a volume has no more blocks than entries
  if (P.voxels && slots > 0)
  {
    hipLaunchKernelGGL(pack_gather_kernel, dim3((slots + waves_per_group - 1) / waves_per_group), dim3(kWaveThreads), 0, s, P);
    VK_LAUNCH_CHECK();
  }
  return VK_OK;
}

size_t vk_volume_merge_packed_workspace_bytes(int32_t block_count)
{
  if (block_count < 0) return 0;
  return merge_workspace_bytes((size_t)block_count);
}

int vk_volume_merge_packed(const vk_volume* dst, const vk_block_pack* pack, int32_t block_count, float voxel_length,
    float truncation_length, const vk_merge_params* p, int32_t* counts_dev, void* workspace, void* stream)
{
  VK_REQUIRE(dst && pack && p && counts_dev && workspace);
  VK_REQUIRE(volume_ok(dst) && merge_params_ok(*p));
  VK_REQUIRE(pack->origins && pack->voxels && aligned(pack->origins, 8) && aligned(pack->voxels, 16) && pack->voxels != dst->voxels);
  VK_REQUIRE(memcmp(&dst->voxel_length, &voxel_length, sizeof(float)) == 0 &&
             memcmp(&dst->truncation_length, &truncation_length, sizeof(float)) == 0);
  VK_REQUIRE(pack->capacity >= 0 && block_count >= 0 && block_count <= pack->capacity);
  hipStream_t s = vk_s(stream);
  PackMerge P;
  P.dst = *dst;
  P.src.origins = pack->origins;
  P.src.voxels = pack->voxels;
  P.src.blocks = block_count;
  P.flags = p->flags;
  P.cap_distance = p->max_distance_weight;
  P.cap_color = p->max_color_weight;
  P.dst_total = dst->main_block_count + dst->excess_block_count;
  merge_carve_workspace(P, workspace);
  P.counts = counts_dev;

  VK_CHECK(hipMemsetAsync(P.ctl, 0, cWords * sizeof(int32_t), s));
  if (block_count == 0)
  {
    // a source without blocks: the six counts are the zero control words, and "afterwards"
    hipLaunchKernelGGL(merge_finish_kernel<PackSource>, dim3(1), dim3(1), 0, s, P);
    VK_LAUNCH_CHECK();
    return VK_OK;
  }
  hipLaunchKernelGGL(merge_init_kernel<PackSource>, dim3((block_count + 255) / 256), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  return merge_enqueue_passes(dst, p, P, stream);
}

}  // extern "C"
