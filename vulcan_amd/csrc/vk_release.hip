// vk_release.hip — give voxel blocks back: release by rule, compact the hash table, rebuild the free list, for gfx950
// (ref: src/volume.cu:304-368 HandleAllocationRequests only ever TAKES a slot and an excess entry; there is no upstream
// counterpart. The definition is in include/vk.h at vk_volume_release_blocks; tests/release_reference.py states it on
// the CPU and the device is held to it bit for bit).
//
// Shape: everything is enqueued on the caller's stream, nothing is read back, and no result depends on the order in which
// workgroups or atomics arrive — every position comes out of an ordered scan (the pattern of vk_extract.hip).
//   snapshot  the table and the visibility bytes as the call found them (new excess positions overlap old ones)
//   mark      one thread per main bucket walks its chain and marks the entries that hold a block
//   classify  one wave per marked entry streams the block's 10 240 bytes once, decides, and — when the block goes —
//             overwrites it with Voxel::Empty() right away: the only pass over the voxel pool
//   count     one thread per main bucket counts its chain's survivors
//   scan      ordered exclusive scan of max(survivors - 1, 0) over the buckets = first excess entry of each
//             (vk_compact_offsets: three launches, stable, any number of buckets)
//   reset     every entry becomes HashEntry(), every visibility byte FALSE
//   rewrite   one thread per main bucket writes its survivors (from the copy of the old table) to their new entries
//   free list the same scan over the unreferenced pool slots, then each writes itself to its position; the -1 tail,
//             the counters
#include "vk_common.hpp"

using namespace vk;

namespace
{

constexpr int kBlockBytes = VK_BLOCK_VOXELS * (int)sizeof(vk_voxel);   // 10 240
constexpr int kBlockVectors = kBlockBytes / 16;                        // 640 16-byte vectors
constexpr int kVectorTrips = kBlockVectors / kWave;                    // 10 per lane
constexpr int kClassifyThreads = 256;                                  // four waves = four entries per workgroup
static_assert(sizeof(vk_voxel) == 20 && kBlockVectors % kWave == 0, "Voxel layout");

struct ReleaseParams
{
  vk_volume v;
  vk_release_rule rule;
  int total;                    // main + excess entries = pool slots
  // workspace
  vk_hash_entry* old_entries;   // [total]  the table as the call found it
  uint8_t* old_visibility;      // [total]
  uint8_t* state;               // [total]  per OLD entry index: kNone, kBlock (marked, undecided), kKeep, kDrop
  int32_t* slot_free;           // [total]  1: no survivor references the pool slot
  int32_t* slot_offset;         // [total]  position of a free slot in the free list (exclusive scan of slot_free)
  int32_t* bucket_kept;         // [main]   survivors of the bucket's chain
  int32_t* bucket_extra;        // [main]   max(survivors - 1, 0)
  int32_t* bucket_first;        // [main]   first excess entry of the bucket's survivors, relative to main (scan of bucket_extra)
  int32_t* totals;              // [4]      kTotal*
  int32_t* counts;              // [4]      output: released, kept, excess entries in use, free slots
};

enum : uint8_t { kNone = 0, kBlock = 1, kKeep = 2, kDrop = 3 };
enum { kTotalExcess = 0, kTotalKept, kTotalDropped, kTotalFree };

// A chain as the release sees it: entry `bucket` first, then along `next`; a link that leaves the table ends it and no
// chain is longer than the table (find_slot's guard, vk_extract.hip — a cycle in a table handed in from outside must not hang).
template <typename F>
__device__ __forceinline__ void walk_chain(const vk_hash_entry* entries, int bucket, int total, F visit)
{
  int index = bucket;
  for (int guard = 0; index >= 0 && index < total && guard < total; ++guard)
  {
    const Entry entry = load_entry(entries, (uint32_t)index);
    visit(index, entry);
    index = entry.next;
  }
}

// new excess positions overlap old ones: everything later reads the table and the visibility bytes from this copy
__global__ __launch_bounds__(256) void snapshot_kernel(ReleaseParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= P.total) return;
  reinterpret_cast<int4*>(P.old_entries)[index] = reinterpret_cast<const int4*>(P.v.hash_entries)[index];
  P.old_visibility[index] = P.v.block_visibility[index];
  P.state[index] = kNone;
  P.slot_free[index] = 1;
  if (index == 0) P.totals[0] = P.totals[1] = P.totals[2] = P.totals[3] = 0;
}

__global__ __launch_bounds__(256) void mark_kernel(ReleaseParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  if (bucket >= P.v.main_block_count) return;
  walk_chain(P.old_entries, bucket, P.total, [&](int index, const Entry& entry) {
    if (entry.data >= 0 && entry.data < P.total) P.state[index] = kBlock;
  });
}

// Dword j of a block belongs to field j % 5 of voxel j / 5 (20-byte AoS voxels): field 0 is the distance, the low half
// of field 4 the distance weight. Lane l of trip t holds vector q = 64 t + l, dwords 4 q .. 4 q + 3.
__device__ __forceinline__ uint32_t empty_dword(int j) { return (j % 5 == 0) ? 0x3f800000u : 0u; }   // Voxel::Empty(): distance 1

// One wave per entry. The decision compares stored values only (vk.h): origin against the box, weights against 0,
// |distance| against the threshold.
__global__ __launch_bounds__(kClassifyThreads) void classify_kernel(ReleaseParams P)
{
  const int index = blockIdx.x * (kClassifyThreads / kWave) + (int)(threadIdx.x >> 6);
  if (index >= P.total) return;
  if (P.state[index] != kBlock) return;          // unallocated, a ghost, or not in any chain: its voxels are never read
  const Entry entry = load_entry(P.old_entries, (uint32_t)index);
  const int lane = lane_id();
  const int flags = P.rule.flags;

  bool drop = false;
  if (flags & VK_RELEASE_OUTSIDE_BOX)
    drop = entry.ox < P.rule.keep_lo[0] || entry.ox > P.rule.keep_hi[0] || entry.oy < P.rule.keep_lo[1] ||
           entry.oy > P.rule.keep_hi[1] || entry.oz < P.rule.keep_lo[2] || entry.oz > P.rule.keep_hi[2];

  uint4* block = reinterpret_cast<uint4*>(reinterpret_cast<char*>(P.v.voxels) + (size_t)entry.data * kBlockBytes);
  if (!drop && (flags & (VK_RELEASE_UNOBSERVED | VK_RELEASE_NO_SURFACE)))
  {
    // the whole block in flight at once: ten coalesced 16-byte loads per lane
    uint4 data[kVectorTrips];
#pragma unroll
    for (int t = 0; t < kVectorTrips; ++t) data[t] = block[t * kWave + lane];

    // a voxel's weight sits four dwords behind its distance: the same component of the NEXT vector, which the next lane
    // holds (lane 63: lane 0 of the next trip; the last vector of a block starts no voxel)
    const float threshold = P.rule.min_abs_distance;
    bool observed = false, near = false;
#pragma unroll
    for (int t = 0; t < kVectorTrips; ++t)
    {
      const uint32_t here[4] = {data[t].x, data[t].y, data[t].z, data[t].w};
      const uint4 wrap = data[t + 1 < kVectorTrips ? t + 1 : t];
      const uint32_t ahead[4] = {wrap.x, wrap.y, wrap.z, wrap.w};
      const int first = 4 * (t * kWave + lane);
#pragma unroll
      for (int c = 0; c < 4; ++c)
      {
        const uint32_t next_lane = (uint32_t)__shfl_down((int)here[c], 1);
        const uint32_t next_trip = (uint32_t)__shfl((int)ahead[c], 0);
        const uint32_t weight_word = (lane == kWave - 1) ? next_trip : next_lane;
        if ((first + c) % 5 == 0)
        {
          const bool seen = (weight_word & 0xffffu) != 0u;          // distance_weight != 0
          observed = observed || seen;
          near = near || (seen && fabsf(__uint_as_float(here[c])) < threshold);
        }
      }
    }
    const bool any_observed = __any(observed ? 1 : 0) != 0;
    const bool any_near = __any(near ? 1 : 0) != 0;
    if ((flags & VK_RELEASE_UNOBSERVED) && !any_observed) drop = true;
    if ((flags & VK_RELEASE_NO_SURFACE) && any_observed && !any_near) drop = true;
  }

  if (drop)
  {
#pragma unroll
    for (int t = 0; t < kVectorTrips; ++t)
    {
      const int first = 4 * (t * kWave + lane);
      block[t * kWave + lane] = make_uint4(empty_dword(first), empty_dword(first + 1), empty_dword(first + 2), empty_dword(first + 3));
    }
  }
  if (lane == 0) P.state[index] = drop ? kDrop : kKeep;
}

// survivors of each bucket; the two sums are integer atomics (they commute: the totals do not depend on arrival order)
__global__ __launch_bounds__(256) void count_kernel(ReleaseParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  int kept = 0, dropped = 0;
  if (bucket < P.v.main_block_count)
  {
    walk_chain(P.old_entries, bucket, P.total, [&](int index, const Entry&) {
      const uint8_t s = P.state[index];
      kept += s == kKeep ? 1 : 0;
      dropped += s == kDrop ? 1 : 0;
    });
    P.bucket_kept[bucket] = kept;
    P.bucket_extra[bucket] = kept > 1 ? kept - 1 : 0;     // survivors that need an excess entry
  }
  // one pair of global atomics per workgroup
  __shared__ int group_sums[2];
  if (threadIdx.x < 2) group_sums[threadIdx.x] = 0;
  __syncthreads();
  for (int d = 32; d > 0; d >>= 1)
  {
    kept += __shfl_down(kept, d);
    dropped += __shfl_down(dropped, d);
  }
  if (lane_id() == 0)
  {
    if (kept) atomicAdd(&group_sums[0], kept);
    if (dropped) atomicAdd(&group_sums[1], dropped);
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    if (group_sums[0]) atomicAdd(&P.totals[kTotalKept], group_sums[0]);
    if (group_sums[1]) atomicAdd(&P.totals[kTotalDropped], group_sums[1]);
  }
}

__global__ __launch_bounds__(256) void reset_kernel(ReleaseParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= P.total) return;
  reinterpret_cast<int4*>(P.v.hash_entries)[index] = make_int4(0, 0, -1, -1);      // HashEntry(): hash.h:18-22
  P.v.block_visibility[index] = VK_VISIBILITY_FALSE;
}

__global__ __launch_bounds__(256) void rewrite_kernel(ReleaseParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  if (bucket >= P.v.main_block_count) return;
  const int survivors = P.bucket_kept[bucket];
  if (survivors == 0) return;
  const int first_excess = P.v.main_block_count + P.bucket_first[bucket];
  int k = 0;
  walk_chain(P.old_entries, bucket, P.total, [&](int index, const Entry& entry) {
    if (P.state[index] != kKeep || k >= survivors) return;
    const int where = k == 0 ? bucket : first_excess + k - 1;
    const int next = k + 1 < survivors ? first_excess + k : -1;
    if (where < P.total)            // (always, for a table whose chains share no entry)
    {
      const int4 raw = reinterpret_cast<const int4*>(P.old_entries)[index];
      reinterpret_cast<int4*>(P.v.hash_entries)[where] = make_int4(raw.x, raw.y, raw.z, next < P.total ? next : -1);
      P.v.block_visibility[where] = P.old_visibility[index];
      P.slot_free[entry.data] = 0;
    }
    ++k;
  });
}

// free_voxel_blocks[k] = the k-th unreferenced slot, ascending (its position is slot_offset, from the ordered scan);
// -1 behind them; the counters
__global__ __launch_bounds__(256) void free_list_kernel(ReleaseParams P)
{
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= P.total) return;
  const int free_slots = P.totals[kTotalFree];
  if (P.slot_free[slot]) P.v.free_voxel_blocks[P.slot_offset[slot]] = slot;
  if (slot >= free_slots) P.v.free_voxel_blocks[slot] = -1;       // (positions below are the free slots' own)
  if (slot == 0)
  {
    const int in_excess = P.totals[kTotalExcess];
    P.v.counters[VK_CTR_VOXEL_PTR] = free_slots - 1;
    P.v.counters[VK_CTR_EXCESS_PTR] = P.v.main_block_count + in_excess;
    P.v.counters[VK_CTR_VISIBLE] = 0;
    P.v.counters[VK_CTR_BANDED] = -1;           // the banded lists list nothing any more
    P.counts[0] = P.totals[kTotalDropped];
    P.counts[1] = P.totals[kTotalKept];
    P.counts[2] = in_excess;
    P.counts[3] = free_slots;
  }
}

}  // namespace

extern "C" {

size_t vk_volume_release_workspace_bytes(int32_t main_block_count, int32_t excess_block_count)
{
  if (main_block_count <= 0 || excess_block_count < 0) return 0;
  const size_t total = (size_t)main_block_count + (size_t)excess_block_count;
  if (total > (size_t)INT32_MAX) return 0;
  return align_up(total * sizeof(vk_hash_entry)) + 2 * align_up(total) + 2 * align_up(total * 4) +
         3 * align_up((size_t)main_block_count * 4) + align_up(16) + align_up(vk_compact_workspace_bytes((int32_t)total));
}

int vk_volume_release_blocks(const vk_volume* v, const vk_release_rule* rule, int32_t* counts_dev, void* workspace, void* stream)
{
  VK_REQUIRE(v && rule && counts_dev && workspace);
  VK_REQUIRE(v->voxels && v->hash_entries && v->free_voxel_blocks && v->block_visibility && v->counters);
  VK_REQUIRE(v->main_block_count > 0 && v->excess_block_count >= 0 && v->excess_block_count <= INT32_MAX - v->main_block_count);
  VK_REQUIRE((rule->flags & ~(VK_RELEASE_UNOBSERVED | VK_RELEASE_NO_SURFACE | VK_RELEASE_OUTSIDE_BOX)) == 0);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(v->voxels) & 15) == 0);      // the pool is streamed in 16-byte vectors
  hipStream_t s = vk_s(stream);
  ReleaseParams P;
  P.v = *v;
  P.rule = *rule;
  P.total = v->main_block_count + v->excess_block_count;
  const size_t total = (size_t)P.total, main = (size_t)v->main_block_count;
  char* at = static_cast<char*>(workspace);
  P.old_entries = reinterpret_cast<vk_hash_entry*>(at);   at += align_up(total * sizeof(vk_hash_entry));
  P.old_visibility = reinterpret_cast<uint8_t*>(at);      at += align_up(total);
  P.state = reinterpret_cast<uint8_t*>(at);               at += align_up(total);
  P.slot_free = reinterpret_cast<int32_t*>(at);           at += align_up(total * 4);
  P.slot_offset = reinterpret_cast<int32_t*>(at);         at += align_up(total * 4);
  P.bucket_kept = reinterpret_cast<int32_t*>(at);         at += align_up(main * 4);
  P.bucket_extra = reinterpret_cast<int32_t*>(at);        at += align_up(main * 4);
  P.bucket_first = reinterpret_cast<int32_t*>(at);        at += align_up(main * 4);
  P.totals = reinterpret_cast<int32_t*>(at);              at += align_up(16);
  void* scan_workspace = at;                              // vk_compact_offsets', used by one scan after the other
  P.counts = counts_dev;

  const int bucket_groups = (v->main_block_count + 255) / 256, entry_groups = (P.total + 255) / 256;
  hipLaunchKernelGGL(snapshot_kernel, dim3(entry_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(mark_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(classify_kernel, dim3((P.total + 3) / 4), dim3(kClassifyThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(count_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  // (a bucket without a survivor in an excess entry gets -1: its bucket_first is never read)
  int code = vk_compact_offsets(P.bucket_extra, v->main_block_count, P.bucket_first, &P.totals[kTotalExcess], scan_workspace, stream);
  if (code != VK_OK) return code;
  hipLaunchKernelGGL(reset_kernel, dim3(entry_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(rewrite_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  code = vk_compact_offsets(P.slot_free, P.total, P.slot_offset, &P.totals[kTotalFree], scan_workspace, stream);
  if (code != VK_OK) return code;
  hipLaunchKernelGGL(free_list_kernel, dim3(entry_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // extern "C"
