// vk_merge_passes.hpp — the passes of vk_volume_merge over "the considered source blocks", written once for the two
// places a source block can come from: an entry of a source volume's table (vk_merge.hip, VolumeSource) and block k of
// a vk_block_pack (vk_pack.hip, PackSource). The definition is in include/vk.h at vk_volume_merge; both entry points
// compile the same float sequence from here, so what they leave is the same bit for bit. Also the two pieces the pack
// side shares with them: a block as 640 16-byte vectors of a wave, and merge's test of a block nobody observed.
//
// A Source is a small struct passed by value in the launch arguments:
//   kListed          true: items 0 .. count()-1 ARE the source blocks (a pack); false: a mark pass names them (a table)
//   count()          items: table entries, or packed blocks
//   origin(i)        item i's block origin, as an Entry's ox, oy, oz
//   block(i)         item i's 512 voxels as 16-byte vectors
#pragma once

#include "vk_alloc_rounds.hpp"

namespace vk
{

constexpr int kBlockBytes = VK_BLOCK_VOXELS * (int)sizeof(vk_voxel);   // 10 240
constexpr int kBlockVectors = kBlockBytes / 16;                        // 640 16-byte vectors
constexpr int kVectorTrips = kBlockVectors / kWave;                    // 10 per lane
constexpr int kWaveThreads = 256;                                      // four waves = four blocks per workgroup
static_assert(sizeof(vk_voxel) == 20 && kBlockVectors % kWave == 0, "Voxel layout");

__device__ __forceinline__ const uint4* pool_block(const vk_voxel* pool, int slot)
{
  return reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(pool) + (size_t)slot * kBlockBytes);
}
__device__ __forceinline__ uint4* pool_block(vk_voxel* pool, int slot)
{
  return reinterpret_cast<uint4*>(reinterpret_cast<char*>(pool) + (size_t)slot * kBlockBytes);
}

// One wave: has a voxel of the block a weight? A block is unobserved when all 512 voxels have both weights 0, i.e. when
// every fifth dword of the block is 0 (dword j is field j % 5 of voxel j / 5, field 4 the two weights). The same answer
// in every lane.
__device__ __forceinline__ bool wave_block_observed(const uint4* block)
{
  const int lane = lane_id();
  uint4 data[kVectorTrips];
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t) data[t] = block[t * kWave + lane];
  uint32_t weights = 0u;
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t)
  {
    const int first = 4 * (t * kWave + lane);
    const uint32_t here[4] = {data[t].x, data[t].y, data[t].z, data[t].w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((first + c) % 5 == 4) weights |= here[c];
  }
  return __any(weights != 0u ? 1 : 0) != 0;
}

enum : uint8_t { kNone = 0, kConsidered = 1, kSkipped = 2, kFusedEarlier = 3 };
// the words that carry the sums, behind the ones that steer the rounds
enum { cConsidered = cRoundWords, cSkipped, cPresentBefore, cPresent, cWords = 16 };

template <class Source>
struct MergeParams
{
  vk_volume dst;
  Source src;
  int flags;
  float cap_distance, cap_color;
  int dst_total;                // main + excess entries = pool slots
  // workspace
  uint8_t* state;               // [src.count()]  kNone, kConsidered, kSkipped, kFusedEarlier
  int32_t* found;               // [src.count()]  pool slot of the block in dst, -1 while it has none
  int32_t* ctl;                 // [cWords]
  int32_t* counts;              // [6] output
};

// (the control words are zero: a memset in front of this launch)
template <class Source>
__global__ __launch_bounds__(256) void merge_init_kernel(MergeParams<Source> P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  int still = 0;
  if (index < P.src.count())
  {
    if (P.flags & VK_MERGE_CONTINUE)
    {
      // the workspace is the previous call's: what that call fused is not fused again, what it left out is what remains
      const uint8_t s = P.state[index];
      if (s == kConsidered && P.found[index] >= 0) P.state[index] = kFusedEarlier;
      still = (s == kConsidered && P.found[index] < 0) ? 1 : 0;
    }
    else
    {
      P.state[index] = Source::kListed ? kConsidered : kNone;
      P.found[index] = -1;
      still = (Source::kListed && !(P.flags & VK_MERGE_SKIP_UNOBSERVED)) ? 1 : 0;   // (classify counts otherwise)
    }
  }
  if (Source::kListed || (P.flags & VK_MERGE_CONTINUE)) wave_add(&P.ctl[cConsidered], still);
  if (index == 0) rounds_begin(P.ctl, P.dst.counters);
}

// SKIP_UNOBSERVED: one wave per considered item; the block is ignored when nobody observed it (wave_block_observed)
template <class Source>
__global__ __launch_bounds__(kWaveThreads) void merge_classify_kernel(MergeParams<Source> P)
{
  const int index = blockIdx.x * (kWaveThreads / kWave) + (int)(threadIdx.x >> 6);
  if (index >= P.src.count()) return;
  if (P.state[index] != kConsidered) return;
  const bool observed = wave_block_observed(P.src.block(index));
  if (lane_id() == 0)
  {
    if (!observed) P.state[index] = kSkipped;
    atomicAdd(&P.ctl[observed ? cConsidered : cSkipped], 1);
  }
}

// One lane per source item. The lane looks for the block in dst (find_block); its slot is kept for the fuse pass. POST: a
// block that is absent asks for a slot (request_block).
template <class Source, bool POST>
__global__ __launch_bounds__(256) void merge_request_kernel(MergeParams<Source> P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (POST && P.ctl[cStop]) return;                   // the rounds are over: this one changes nothing
  int present = 0, posted = 0;
  if (index < P.src.count() && P.state[index] == kConsidered)
  {
    int slot = P.found[index];
    if (slot < 0)
    {
      const Entry mine = P.src.origin(index);
      Entry main_entry;
      find_block(P.dst, P.dst_total, mine.ox, mine.oy, mine.oz, slot, main_entry);
      if (slot >= 0) P.found[index] = slot;
      else if (POST)
      {
        request_block(P.dst, mine.ox, mine.oy, mine.oz, main_entry);
        posted = 1;
      }
    }
    present = slot >= 0 ? 1 : 0;
  }
  if (POST)
  {
    wave_add(&P.ctl[cPosted], posted);
    // the first round of a call sees the blocks that were there before it
    if (P.ctl[cRounds] == 0) wave_add(&P.ctl[cPresentBefore], present);
  }
  else wave_add(&P.ctl[cPresent], present);
}

template <class Source>
__global__ void merge_finish_kernel(MergeParams<Source> P)
{
  const int32_t* ctl = P.ctl;
  P.counts[0] = ctl[cConsidered];
  P.counts[1] = ctl[cPresent];
  P.counts[2] = ctl[cPresent] - ctl[cPresentBefore];
  P.counts[3] = ctl[cConsidered] - ctl[cPresent];
  P.counts[4] = ctl[cRounds];
  P.counts[5] = ctl[cSkipped];
  lists_stale(P.dst.counters);
}

// a[i] of eight values for a lane-dependent i, as selects: an array indexed at run time would leave the registers
__device__ __forceinline__ uint32_t pick8(int i, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4, uint32_t a5,
    uint32_t a6, uint32_t a7)
{
  uint32_t out = a0;
  out = i == 1 ? a1 : out;
  out = i == 2 ? a2 : out;
  out = i == 3 ? a3 : out;
  out = i == 4 ? a4 : out;
  out = i == 5 ? a5 : out;
  out = i == 6 ? a6 : out;
  out = i == 7 ? a7 : out;
  return out;
}

// One wave per source block. Both blocks move as ten coalesced 16-byte loads per lane, the result as ten 16-byte stores.
// Lane l of trip t holds vector q = 64 t + l, dwords 4 q .. 4 q + 3; dword j is field j % 5 of voxel j / 5. What a
// dword becomes depends on itself, on the source's dword in the same place and on the two weight words of its voxel,
// which lie at most four dwords ahead: in the lane's own vector or in the next lane's (lane 63: lane 0 of the next trip;
// the last vector of a block ends with a weight word). No LDS, no atomics: a dst block has one source block.
template <class Source>
__global__ __launch_bounds__(kWaveThreads) void merge_fuse_kernel(MergeParams<Source> P)
{
  const int index = blockIdx.x * (kWaveThreads / kWave) + (int)(threadIdx.x >> 6);
  if (index >= P.src.count()) return;
  if (P.state[index] != kConsidered) return;
  const int slot = P.found[index];
  if (slot < 0) return;                            // left out
  const int lane = lane_id();
  const uint4* src = P.src.block(index);
  uint4* dst = pool_block(P.dst.voxels, slot);

  uint4 s[kVectorTrips], d[kVectorTrips];
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t) s[t] = src[t * kWave + lane];
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t) d[t] = dst[t * kWave + lane];

  const float cap_d = P.cap_distance, cap_c = P.cap_color;
#pragma unroll
  for (int t = 0; t < kVectorTrips; ++t)
  {
    const int tn = t + 1 < kVectorTrips ? t + 1 : t;
    const uint32_t s_here[4] = {s[t].x, s[t].y, s[t].z, s[t].w}, d_here[4] = {d[t].x, d[t].y, d[t].z, d[t].w};
    const uint32_t s_wrap[4] = {s[tn].x, s[tn].y, s[tn].z, s[tn].w}, d_wrap[4] = {d[tn].x, d[tn].y, d[tn].z, d[tn].w};
    uint32_t s_behind[4], d_behind[4];               // the vector behind this lane's
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
      const uint32_t s_next = (uint32_t)__shfl_down((int)s_here[c], 1), d_next = (uint32_t)__shfl_down((int)d_here[c], 1);
      const uint32_t s_trip = (uint32_t)__shfl((int)s_wrap[c], 0), d_trip = (uint32_t)__shfl((int)d_wrap[c], 0);
      s_behind[c] = (lane == kWave - 1) ? s_trip : s_next;
      d_behind[c] = (lane == kWave - 1) ? d_trip : d_next;
    }
    // the weight words of the eight dwords: at offset `first_weight` and five dwords on (if that is still among them)
    const int phase = (4 * (t * kWave + lane)) % 5;             // field of the lane's first dword
    const int first_weight = 4 - phase;
    const uint32_t s_w1 = pick8(first_weight, s_here[0], s_here[1], s_here[2], s_here[3], s_behind[0], s_behind[1], s_behind[2], s_behind[3]);
    const uint32_t d_w1 = pick8(first_weight, d_here[0], d_here[1], d_here[2], d_here[3], d_behind[0], d_behind[1], d_behind[2], d_behind[3]);
    // (read only when first_weight + 5 <= 7: then it is dword first_weight + 1 of the vector behind)
    const uint32_t s_w2 = pick8(first_weight + 1, s_behind[0], s_behind[1], s_behind[2], s_behind[3], 0u, 0u, 0u, 0u);
    const uint32_t d_w2 = pick8(first_weight + 1, d_behind[0], d_behind[1], d_behind[2], d_behind[3], 0u, 0u, 0u, 0u);

    uint32_t out[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
      const int field = (phase + c) % 5;
      const uint32_t s_weights = c <= first_weight ? s_w1 : s_w2, d_weights = c <= first_weight ? d_w1 : d_w2;
      const int16_t s_dw = (int16_t)(s_weights & 0xffffu), s_cw = (int16_t)(s_weights >> 16);
      const int16_t d_dw = (int16_t)(d_weights & 0xffffu), d_cw = (int16_t)(d_weights >> 16);
      // the running average of the field (depth_integrator.cu:55-59, color_integrator.cu:109-118), continued with the
      // source's weight in place of 1: fp32, one rounding per operation
      const int16_t s_weight = field == 0 ? s_dw : s_cw, d_weight = field == 0 ? d_dw : d_cw;
      const float wd = (float)d_weight, ws = (float)s_weight;
      const float sum = wd + ws;
      const float sv = __uint_as_float(s_here[c]), dv = __uint_as_float(d_here[c]);
      const float mean = (wd * dv + ws * sv) / sum;
      const uint32_t value = s_weight == 0 ? d_here[c] : (d_weight == 0 ? s_here[c] : __float_as_uint(mean));
      // the weight word itself (then s_weights is s_here[c])
      const float sum_d = (float)d_dw + (float)s_dw, sum_c = (float)d_cw + (float)s_cw;
      const int16_t new_dw = s_dw == 0 ? d_dw : (int16_t)fminf(cap_d, sum_d);
      const int16_t new_cw = s_cw == 0 ? d_cw : (int16_t)fminf(cap_c, sum_c);
      const uint32_t word = (uint32_t)(uint16_t)new_dw | ((uint32_t)(uint16_t)new_cw << 16);
      out[c] = field == 4 ? word : value;
    }
    dst[t * kWave + lane] = make_uint4(out[0], out[1], out[2], out[3]);
  }
}

// What is enqueued behind the listing of the source blocks (init, and a table's mark pass): classify, the rounds, resolve,
// finish, fuse. `P.src.count()` > 0.
template <class Source>
int merge_enqueue_passes(const vk_volume* dst, const vk_merge_params* p, const MergeParams<Source>& P, void* stream)
{
  hipStream_t s = vk_s(stream);
  const int items = P.src.count();
  const int entry_groups = (items + 255) / 256;
  const int wave_groups = (items + kWaveThreads / kWave - 1) / (kWaveThreads / kWave);
  if ((p->flags & VK_MERGE_SKIP_UNOBSERVED) && !(p->flags & VK_MERGE_CONTINUE))
  {
    hipLaunchKernelGGL(merge_classify_kernel<Source>, dim3(wave_groups), dim3(kWaveThreads), 0, s, P);
    VK_LAUNCH_CHECK();
  }
  const int code = run_rounds(dst, p->max_rounds, P.ctl, stream,
      [&] { hipLaunchKernelGGL((merge_request_kernel<Source, true>), dim3(entry_groups), dim3(256), 0, s, P); });
  if (code != VK_OK) return code;
  hipLaunchKernelGGL((merge_request_kernel<Source, false>), dim3(entry_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(merge_finish_kernel<Source>, dim3(1), dim3(1), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(merge_fuse_kernel<Source>, dim3(wave_groups), dim3(kWaveThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

// the workspace of a merge over `items` source items: state, found, the control words
inline size_t merge_workspace_bytes(size_t items) { return align_up(items) + align_up(items * 4) + align_up(cWords * 4); }

template <class Source>
void merge_carve_workspace(MergeParams<Source>& P, void* workspace)
{
  const size_t items = (size_t)P.src.count();
  char* at = static_cast<char*>(workspace);
  P.state = reinterpret_cast<uint8_t*>(at);       at += align_up(items);
  P.found = reinterpret_cast<int32_t*>(at);       at += align_up(items * 4);
  P.ctl = reinterpret_cast<int32_t*>(at);
}

}  // namespace vk
