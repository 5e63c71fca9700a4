// vk_merge_pose.hip — fuse one voxel-hashed volume into another through a rigid pose, for gfx950
// (no upstream counterpart: its Volume is a process-wide singleton, src/volume.cu:17-21; ref: src/volume.cu:304-368 for
// the allocation, which goes through the existing handle pass, src/depth_integrator.cu:55-59 and
// src/color_integrator.cu:109-118 for the running averages the fusion continues. The definition is in include/vk.h at
// vk_volume_merge_posed; tests/merge_pose_reference.py states it on the CPU and the device is held to it bit for bit).
//
// Shape: everything is enqueued on the caller's stream and nothing is read back. Every decision compares stored or
// computed fp32 values whose operation order is fixed, every count is an integer sum, a bucket's contest is won by the
// largest key and a destination block is written by one wave, so no result depends on the order in which workgroups or
// atomics arrive.
//   init      per source entry and per destination entry: state; the words that steer the rounds
//   mark      one thread per source bucket walks its chain and marks the entries that hold a block
//   classify  (SKIP_UNOBSERVED only) one wave per marked entry drops the block when no voxel has a weight
//   geometry  one wave per considered source block: the block's box in dst and, per block of the box, whether one of
//             its 512 centres falls back into the source block: 27 bits per source entry, independent of dst's table
//   rounds    max_rounds times: request pass (one lane per source entry and box block: the dst chain walk, then the
//             idempotent candidate mark or the request), the existing handle pass, round end
//   resolve   the request pass once more, without posting: marks what the last round allocated, counts what stays absent
//   finish    the eight counts, VK_CTR_VISIBLE and VK_CTR_BANDED
//   fuse      one wave per marked destination entry: the source footprint's slots once into an LDS directory, then the
//             eight-point gather per voxel through it: the only pass over the two voxel pools
#include "vk_alloc_rounds.hpp"

using namespace vk;

namespace
{

constexpr int kWaveThreads = 256;                                      // four waves = four entries per workgroup
constexpr int kWavesPerGroup = kWaveThreads / kWave;
constexpr int kBoxBlocks = 27;                                         // a rigid pose spans at most 3 blocks per axis
constexpr int kLanesPerEntry = 32;                                     // request pass: one lane per box block, 27 of 32
constexpr int kCoordinateClamp = 40000;                                // beyond the int16 range: see block_box

enum : uint8_t { kNone = 0, kConsidered = 1, kSkipped = 2 };            // a source entry
enum : int32_t { kNoCandidate = 0, kCandidate = 1, kFused = 2 };        // a destination entry
// the words that carry the sums, behind the ones that steer the rounds
enum { cConsidered = cRoundWords, cSkipped, cPresentBefore, cMarked, cAbsent, cWords = 16 };

struct PoseParams
{
  vk_volume dst, src;
  int flags;
  float cap_distance, cap_color;
  int dst_total, src_total;     // main + excess entries = pool slots
  float fwd[12], back[12];      // row a: m[a], m[4+a], m[8+a], the translation in voxels
  // workspace
  uint8_t* state;               // [src_total]  kNone, kConsidered, kSkipped
  int4* box;                    // [src_total]  lo of the block's box in dst, and the 27 candidate bits
  int32_t* mark;                // [dst_total]  kNoCandidate, kCandidate, kFused
  int32_t* ctl;                 // [cWords]
  int32_t* counts;              // [8] output
};

__device__ __forceinline__ int block_coordinate(float v)
{
  return vclampi(f2i(floorf(v * 0.125f)), -kCoordinateClamp, kCoordinateClamp);
}

// the blocks [lo, hi]^3 that the eight corners of block (bx, by, bz) reach through `r`, at most three per axis. The
// clamp keeps lo + 2 an int whatever the pose holds; a block beyond it is beyond the int16 range on either side of it.
__device__ __forceinline__ void block_box(const float* r, int bx, int by, int bz, int lo[3], int hi[3])
{
  f3 least = apply(r, (float)(8 * bx), (float)(8 * by), (float)(8 * bz)), most = least;
#pragma unroll
  for (int s = 1; s < 8; ++s)
  {
    const f3 q = apply(r, (float)(8 * bx + 8 * (s & 1)), (float)(8 * by + 8 * ((s >> 1) & 1)), (float)(8 * bz + 8 * (s >> 2)));
    least = f3{fminf(least.x, q.x), fminf(least.y, q.y), fminf(least.z, q.z)};
    most = f3{fmaxf(most.x, q.x), fmaxf(most.y, q.y), fmaxf(most.z, q.z)};
  }
  lo[0] = block_coordinate(least.x);  lo[1] = block_coordinate(least.y);  lo[2] = block_coordinate(least.z);
  hi[0] = vmini(block_coordinate(most.x), lo[0] + 2);
  hi[1] = vmini(block_coordinate(most.y), lo[1] + 2);
  hi[2] = vmini(block_coordinate(most.z), lo[2] + 2);
}

// (the control words are zero: a memset in front of this launch)
__global__ __launch_bounds__(256) void pose_init_kernel(PoseParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  int still = 0;
  if (P.flags & VK_MERGE_CONTINUE)
  {
    // the workspace is the previous call's: the same source blocks, their boxes, and what has been fused already
    if (index < P.src_total) still = P.state[index] == kConsidered ? 1 : 0;
    wave_add(&P.ctl[cConsidered], still);
  }
  else
  {
    if (index < P.src_total) P.state[index] = kNone;
    if (index < P.dst_total) P.mark[index] = kNoCandidate;
  }
  if (index == 0) rounds_begin(P.ctl, P.dst.counters);
}

// one thread per source bucket: its source blocks (mark_chain)
__global__ __launch_bounds__(256) void pose_mark_kernel(PoseParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  const int blocks = mark_chain(P.src, P.src_total, bucket, [&](int index) { P.state[index] = kConsidered; });
  if (!(P.flags & VK_MERGE_SKIP_UNOBSERVED)) wave_add(&P.ctl[cConsidered], blocks);   // (classify counts otherwise)
}

// SKIP_UNOBSERVED: one wave per marked entry; the block is ignored when every voxel's weight word is 0
__global__ __launch_bounds__(kWaveThreads) void pose_classify_kernel(PoseParams P)
{
  const int index = blockIdx.x * kWavesPerGroup + (int)(threadIdx.x >> 6);
  if (index >= P.src_total) return;
  if (P.state[index] != kConsidered) return;
  const Entry entry = load_entry(P.src.hash_entries, (uint32_t)index);
  const int lane = lane_id();
  const uint32_t* block = reinterpret_cast<const uint32_t*>(P.src.voxels) + (size_t)entry.data * VK_BLOCK_VOXELS * kVoxelWords;
  uint32_t weights = 0u;
#pragma unroll
  for (int t = 0; t < VK_BLOCK_VOXELS / kWave; ++t) weights |= block[(size_t)(t * kWave + lane) * kVoxelWords + 4];
  const bool observed = __any(weights != 0u ? 1 : 0) != 0;
  if (lane == 0)
  {
    if (!observed) P.state[index] = kSkipped;
    atomicAdd(&P.ctl[observed ? cConsidered : cSkipped], 1);
  }
}

// One wave per considered source block with origin o. Each block B of o's box in dst sends its 512 centres, eight per
// lane, back into src: B is a candidate of o when one of them lands in a cell of o. One vote per block of the box.
__global__ __launch_bounds__(kWaveThreads) void pose_geometry_kernel(PoseParams P)
{
  const int index = blockIdx.x * kWavesPerGroup + (int)(threadIdx.x >> 6);
  if (index >= P.src_total) return;
  if (P.state[index] != kConsidered) return;
  const Entry mine = load_entry(P.src.hash_entries, (uint32_t)index);
  const int lane = lane_id();
  int lo[3], hi[3];
  block_box(P.fwd, mine.ox, mine.oy, mine.oz, lo, hi);
  const float first_x = (float)(8 * mine.ox), first_y = (float)(8 * mine.oy), first_z = (float)(8 * mine.oz);
  const float last_x = (float)(8 * mine.ox + 7), last_y = (float)(8 * mine.oy + 7), last_z = (float)(8 * mine.oz + 7);
  int bits = 0;
  for (int cell = 0; cell < kBoxBlocks; ++cell)
  {
    const int bx = lo[0] + cell % 3, by = lo[1] + (cell / 3) % 3, bz = lo[2] + cell / 9;
    if (bx > hi[0] || by > hi[1] || bz > hi[2] || !in_int16(bx, by, bz)) continue;       // (the same for the whole wave)
    const float cx = (float)(8 * bx + (lane & 7)) + 0.5f, cy = (float)(8 * by + (lane >> 3)) + 0.5f;
    bool hit = false;
#pragma unroll
    for (int z = 0; z < 8; ++z)
    {
      const f3 p = apply(P.back, cx, cy, (float)(8 * bz + z) + 0.5f);
      const float qx = floorf(p.x), qy = floorf(p.y), qz = floorf(p.z);
      hit = hit || (qx >= first_x && qx <= last_x && qy >= first_y && qy <= last_y && qz >= first_z && qz <= last_z);
    }
    if (__any(hit ? 1 : 0)) bits |= 1 << cell;
  }
  if (lane == 0) P.box[index] = make_int4(lo[0], lo[1], lo[2], bits);
}

// Is source entry `index` the first of the considered source blocks that have block (bx, by, bz) as a candidate? The
// others can only be among the blocks the block's own corners reach through `back`. (Absent candidates have no entry of
// dst to be counted at: each is counted by this one source block.)
__device__ __forceinline__ bool first_owner(const PoseParams& P, int index, int bx, int by, int bz)
{
  int lo[3], hi[3];
  block_box(P.back, bx, by, bz, lo, hi);
  for (int cell = 0; cell < kBoxBlocks; ++cell)
  {
    const int ox = lo[0] + cell % 3, oy = lo[1] + (cell / 3) % 3, oz = lo[2] + cell / 9;
    if (ox > hi[0] || oy > hi[1] || oz > hi[2] || !in_int16(ox, oy, oz)) continue;
    int slot;
    Entry main_entry;
    const int other = find_block(P.src, P.src_total, ox, oy, oz, slot, main_entry);
    if (other < 0 || other >= index || P.state[other] != kConsidered) continue;
    const int4 box = P.box[other];
    const int rx = bx - box.x, ry = by - box.y, rz = bz - box.z;
    if (rx < 0 || rx > 2 || ry < 0 || ry > 2 || rz < 0 || rz > 2) continue;
    if ((box.w >> (rx + 3 * ry + 9 * rz)) & 1) return false;
  }
  return true;
}

// One lane per source entry and block of its box. The lane walks the chain of the candidate's bucket in dst. A candidate
// that is there is marked at its entry, once (the compare-and-swap decides who counts it; a mark of an earlier call
// stays). POST: one that is absent asks for a slot (request_block).
template <bool POST>
__global__ __launch_bounds__(256) void pose_request_kernel(PoseParams P)
{
  const long long thread = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int index = (int)(thread / kLanesPerEntry), cell = (int)(thread % kLanesPerEntry);
  if (POST && P.ctl[cStop]) return;                   // the rounds are over: this one changes nothing
  int marked = 0, posted = 0, absent = 0;
  if (index < P.src_total && cell < kBoxBlocks && P.state[index] == kConsidered)
  {
    const int4 box = P.box[index];
    if ((box.w >> cell) & 1)
    {
      const int bx = box.x + cell % 3, by = box.y + (cell / 3) % 3, bz = box.z + cell / 9;
      int slot;
      Entry main_entry;
      const int at = find_block(P.dst, P.dst_total, bx, by, bz, slot, main_entry);
      if (at >= 0)
      {
        if (P.mark[at] == kNoCandidate) marked = atomicCAS(&P.mark[at], (int32_t)kNoCandidate, (int32_t)kCandidate) == kNoCandidate ? 1 : 0;
      }
      else if (POST)
      {
        request_block(P.dst, bx, by, bz, main_entry);
        posted = 1;
      }
      else absent = first_owner(P, index, bx, by, bz) ? 1 : 0;
    }
  }
  wave_add(&P.ctl[cMarked], marked);
  if (POST)
  {
    wave_add(&P.ctl[cPosted], posted);
    // the first round of a call marks the candidates that were there before it
    if (P.ctl[cRounds] == 0) wave_add(&P.ctl[cPresentBefore], marked);
  }
  else wave_add(&P.ctl[cAbsent], absent);
}

__global__ void pose_finish_kernel(PoseParams P)
{
  const int32_t* ctl = P.ctl;
  P.counts[0] = ctl[cConsidered];
  P.counts[1] = ctl[cMarked] + ctl[cAbsent];
  P.counts[2] = ctl[cMarked];
  P.counts[3] = ctl[cMarked] - ctl[cPresentBefore];
  P.counts[4] = ctl[cAbsent];
  P.counts[5] = ctl[cRounds];
  P.counts[6] = ctl[cSkipped];
  P.counts[7] = 0;                              // the fuse pass adds to it
  lists_stale(P.dst.counters);
}

// One wave per marked dst entry, eight voxels per lane (lane = 8 y + x, one z per trip). The source footprint's slots go
// into the wave's LDS directory once (fill_directory), so a voxel's eight neighbours cost eight pool reads and no table
// read. A lattice point outside the directory (no rigid pose gets there) counts as absent.
__global__ __launch_bounds__(kWaveThreads) void pose_fuse_kernel(PoseParams P)
{
  __shared__ int directory[kWavesPerGroup][kWave];
  const int wave = (int)(threadIdx.x >> 6);
  const int at = blockIdx.x * kWavesPerGroup + wave;
  if (at >= P.dst_total) return;
  if (P.mark[at] != kCandidate) return;
  const Entry mine = load_entry(P.dst.hash_entries, (uint32_t)at);
  if (mine.data < 0 || mine.data >= P.dst_total) return;
  const int lane = lane_id();
  const int x = lane & 7, y = lane >> 3;

  int least_x, least_y, least_z;
  fill_directory(P.src, P.src_total, P.back, mine, directory[wave], least_x, least_y, least_z);

  const uint32_t* src_pool = reinterpret_cast<const uint32_t*>(P.src.voxels);
  uint32_t* mine_voxels = reinterpret_cast<uint32_t*>(P.dst.voxels) + (size_t)mine.data * VK_BLOCK_VOXELS * kVoxelWords;
  const float cap_d = P.cap_distance, cap_c = P.cap_color;
  int sampled = 0;
#pragma unroll 1
  for (int z = 0; z < 8; ++z)
  {
    const Lattice l = lattice_of(P.back, mine.ox, mine.oy, mine.oz, x, y, z);
    const bool far_x = l.fx != 0.0f, far_y = l.fy != 0.0f, far_z = l.fz != 0.0f;
    float distance[8], red[8], green[8], blue[8];
    bool has_d = true, has_c = true;
    int least_dw = 32767, least_cw = 32767;
#pragma unroll
    for (int s = 0; s < 8; ++s)
    {
      distance[s] = red[s] = green[s] = blue[s] = 0.0f;
      const bool used = (!(s & 1) || far_x) && (!(s & 2) || far_y) && (!(s & 4) || far_z);
      if (!used) continue;
      const int nx = l.bx + (s & 1), ny = l.by + ((s >> 1) & 1), nz = l.bz + (s >> 2);
      const int rx = (nx >> 3) - least_x, ry = (ny >> 3) - least_y, rz = (nz >> 3) - least_z;
      int slot = -1;
      if (rx >= 0 && rx < kFootprint && ry >= 0 && ry < kFootprint && rz >= 0 && rz < kFootprint)
        slot = directory[wave][rx + kFootprint * ry + kFootprint * kFootprint * rz];
      if (slot < 0)
      {
        has_d = has_c = false;
        continue;
      }
      const uint32_t* voxel = src_pool + ((size_t)slot * VK_BLOCK_VOXELS + (size_t)((nz & 7) * 64 + (ny & 7) * 8 + (nx & 7))) * kVoxelWords;
      const vu4 head = *reinterpret_cast<const vu4*>(voxel);
      const uint32_t weights = voxel[4];
      const int dw = (int16_t)(weights & 0xffffu), cw = (int16_t)(weights >> 16);
      distance[s] = __uint_as_float(head.x);
      red[s] = __uint_as_float(head.y);
      green[s] = __uint_as_float(head.z);
      blue[s] = __uint_as_float(head.w);
      has_d = has_d && dw != 0;
      has_c = has_c && cw != 0;
      least_dw = vmini(least_dw, dw);
      least_cw = vmini(least_cw, cw);
    }
    if (has_d || has_c)
    {
      uint32_t* voxel = mine_voxels + (size_t)(z * 64 + lane) * kVoxelWords;
      const vu4 head = *reinterpret_cast<const vu4*>(voxel);
      const uint32_t weights = voxel[4];
      int16_t dw = (int16_t)(weights & 0xffffu), cw = (int16_t)(weights >> 16);
      uint32_t out[4] = {head.x, head.y, head.z, head.w};
      // the running average of the field (depth_integrator.cu:55-59, color_integrator.cu:109-118), continued with the
      // sample's weight in place of 1: fp32, one rounding per operation
      if (has_d)
      {
        const float sample = trilinear(distance, l.fx, l.fy, l.fz);
        const float wd = (float)dw, ws = (float)least_dw, sum = wd + ws;
        const float mean = (wd * __uint_as_float(out[0]) + ws * sample) / sum;
        out[0] = dw == 0 ? __float_as_uint(sample) : __float_as_uint(mean);
        dw = (int16_t)fminf(cap_d, sum);
        ++sampled;
      }
      if (has_c)
      {
        const float samples[3] = {trilinear(red, l.fx, l.fy, l.fz), trilinear(green, l.fx, l.fy, l.fz), trilinear(blue, l.fx, l.fy, l.fz)};
        const float wd = (float)cw, ws = (float)least_cw, sum = wd + ws;
#pragma unroll
        for (int c = 0; c < 3; ++c)
        {
          const float mean = (wd * __uint_as_float(out[1 + c]) + ws * samples[c]) / sum;
          out[1 + c] = cw == 0 ? __float_as_uint(samples[c]) : __float_as_uint(mean);
        }
        cw = (int16_t)fminf(cap_c, sum);
      }
      vu4 stored;
      stored.x = out[0];  stored.y = out[1];  stored.z = out[2];  stored.w = out[3];
      *reinterpret_cast<vu4*>(voxel) = stored;
      voxel[4] = (uint32_t)(uint16_t)dw | ((uint32_t)(uint16_t)cw << 16);
    }
  }
  wave_add(&P.counts[7], sampled);
  if (lane == 0) P.mark[at] = kFused;            // a call that continues passes over it
}

}  // namespace

extern "C" {

size_t vk_volume_merge_posed_workspace_bytes(int32_t src_main, int32_t src_excess, int32_t dst_main, int32_t dst_excess)
{
  if (src_main <= 0 || src_excess < 0 || dst_main <= 0 || dst_excess < 0) return 0;
  const size_t src_total = (size_t)src_main + (size_t)src_excess, dst_total = (size_t)dst_main + (size_t)dst_excess;
  if (src_total > (size_t)INT32_MAX || dst_total > (size_t)INT32_MAX) return 0;
  return align_up(src_total) + align_up(src_total * sizeof(int4)) + align_up(dst_total * 4) + align_up(cWords * 4);
}

int vk_volume_merge_posed(const vk_volume* dst, const vk_volume* src, const vk_merge_pose_params* p, int32_t* counts_dev,
    void* workspace, void* stream)
{
  VK_REQUIRE(dst && src && p && counts_dev && workspace);
  const vk_merge_params& m = p->merge;
  VK_REQUIRE(merge_ok(dst, src, m));
  PoseParams P;
  VK_REQUIRE(voxel_rows(p->pose.m, dst->voxel_length, P.fwd) && voxel_rows(p->pose.inv, dst->voxel_length, P.back));
  hipStream_t s = vk_s(stream);
  P.dst = *dst;
  P.src = *src;
  P.flags = m.flags;
  P.cap_distance = m.max_distance_weight;
  P.cap_color = m.max_color_weight;
  P.dst_total = dst->main_block_count + dst->excess_block_count;
  P.src_total = src->main_block_count + src->excess_block_count;
  const size_t src_total = (size_t)P.src_total, dst_total = (size_t)P.dst_total;
  char* at = static_cast<char*>(workspace);
  P.state = reinterpret_cast<uint8_t*>(at);       at += align_up(src_total);
  P.box = reinterpret_cast<int4*>(at);            at += align_up(src_total * sizeof(int4));
  P.mark = reinterpret_cast<int32_t*>(at);        at += align_up(dst_total * 4);
  P.ctl = reinterpret_cast<int32_t*>(at);
  P.counts = counts_dev;

  const int most = P.src_total > P.dst_total ? P.src_total : P.dst_total;
  const int bucket_groups = (src->main_block_count + 255) / 256, init_groups = (most + 255) / 256;
  const int src_wave_groups = (P.src_total + kWavesPerGroup - 1) / kWavesPerGroup;
  const int dst_wave_groups = (P.dst_total + kWavesPerGroup - 1) / kWavesPerGroup;
  const long long request_groups = ((long long)P.src_total * kLanesPerEntry + 255) / 256;
  VK_REQUIRE(request_groups <= (long long)INT32_MAX);
  VK_CHECK(hipMemsetAsync(P.ctl, 0, cWords * sizeof(int32_t), s));
  hipLaunchKernelGGL(pose_init_kernel, dim3(init_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  if (!(m.flags & VK_MERGE_CONTINUE))
  {
    hipLaunchKernelGGL(pose_mark_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
    VK_LAUNCH_CHECK();
    if (m.flags & VK_MERGE_SKIP_UNOBSERVED)
    {
      hipLaunchKernelGGL(pose_classify_kernel, dim3(src_wave_groups), dim3(kWaveThreads), 0, s, P);
      VK_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pose_geometry_kernel, dim3(src_wave_groups), dim3(kWaveThreads), 0, s, P);
    VK_LAUNCH_CHECK();
  }
  const int code = run_rounds(dst, m.max_rounds, P.ctl, stream,
      [&] { hipLaunchKernelGGL(pose_request_kernel<true>, dim3((unsigned)request_groups), dim3(256), 0, s, P); });
  if (code != VK_OK) return code;
  hipLaunchKernelGGL(pose_request_kernel<false>, dim3((unsigned)request_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(pose_finish_kernel, dim3(1), dim3(1), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(pose_fuse_kernel, dim3(dst_wave_groups), dim3(kWaveThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // extern "C"
