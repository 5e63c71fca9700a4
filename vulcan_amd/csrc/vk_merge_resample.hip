// vk_merge_resample.hip — fuse one voxel-hashed volume into another of another voxel and truncation length, through a
// rigid pose and a change of scale, for gfx950
// (no upstream counterpart: its Volume is a process-wide singleton, src/volume.cu:17-21; ref: src/volume.cu:304-368 for
// the allocation, which goes through the existing handle pass, src/depth_integrator.cu:55-59 and
// src/color_integrator.cu:109-118 for the running averages the fusion continues and for the band a stored distance lies
// in. The definition is in include/vk.h at vk_volume_merge_resampled; tests/merge_resample_reference.py states it on the
// CPU and the device is held to it bit for bit).
//
// Shape: vk_merge_pose.hip's, with a box of K^3 blocks per source block in the place of 27, n^3 sample points per voxel in
// the place of one and a directory of D^3 blocks per carried block in the place of 64. Everything is enqueued on the
// caller's stream and nothing is read back; no result depends on the order in which workgroups or atomics arrive.
//   init      per source entry and per destination entry: state; the words that steer the rounds
//   mark      one thread per source bucket walks its chain and flags the entries that hold a block
//   classify  (SKIP_UNOBSERVED only) one wave per flagged entry drops the block when no voxel has a weight
//   list      an ordered scan over the flags (vk_compact_offsets), then the considered entries in ascending order: the
//             passes below run over this list and not over the table
//   geometry  one wave per considered source block: the block's box in dst and, per block of the box, whether one of
//             its 512 n^3 sample points falls back into the source block: K^3 bits per source entry
//   rounds    max_rounds times: request pass (one wave per considered entry, the lanes striding over the box: the dst
//             chain walk, then the idempotent candidate mark or the request), the existing handle pass, round end
//   resolve   the request pass once more, without posting: marks what the last round allocated, counts what stays absent
//   finish    the eight counts, VK_CTR_VISIBLE and VK_CTR_BANDED
//   fuse      one wave per marked destination entry: the source footprint's slots once into an LDS directory of D^3
//             cells, then per voxel the n^3 eight-point gathers through it: the only pass over the two voxel pools
#include "vk_alloc_rounds.hpp"

using namespace vk;

namespace
{

constexpr int kWaveThreads = 256;                                      // four waves = four entries per workgroup
constexpr int kWavesPerGroup = kWaveThreads / kWave;
constexpr int kMostBox = 8;                                            // K at a ratio of 4
constexpr int kMostDirectory = 9;                                      // D at a ratio of 1/4
constexpr int kCoordinateClamp = 40000;                                // beyond the int16 range: see block_box
constexpr float kDiagonal = 1.7320508f;                                // of a unit cube

enum : uint8_t { kNone = 0, kConsidered = 1, kSkipped = 2 };            // a source entry
enum : int32_t { kNoCandidate = 0, kCandidate = 1, kFused = 2 };        // a destination entry
// the words that carry the sums, behind the ones that steer the rounds
enum { cConsidered = cRoundWords, cSkipped, cPresentBefore, cMarked, cAbsent, cListed, cWords = 16 };

struct ResampleParams
{
  vk_volume dst, src;
  int flags;
  float cap_distance, cap_color;
  int dst_total, src_total;     // main + excess entries = pool slots
  float fwd[12], back[12];      // row a: the rotation times the ratio of the voxel lengths, the translation in voxels
  float scale;                  // k: a source truncation length in destination truncation lengths
  int rescale;                  // k != 1.0f
  int n, points;                // sample points per axis and per voxel
  int box, box_cells, words;    // K, K^3, the 32-bit words that hold K^3 bits
  int back_box;                 // K of the way back: the source blocks a destination block's corners reach
  int side;                     // D: the directory's blocks per axis
  // workspace
  uint8_t* state;               // [src_total]  kNone, kConsidered, kSkipped
  int32_t* flag;                // [src_total]  1: considered
  int32_t* offset;              // [src_total]  the entry's place in the list
  int32_t* list;                // [src_total]  the considered entries, ascending
  int4* lo;                     // [src_total]  lo of the block's box in dst
  uint32_t* bits;               // [src_total * words]  the candidate bits of the box
  int32_t* mark;                // [dst_total]  kNoCandidate, kCandidate, kFused
  int32_t* ctl;                 // [cWords]
  int32_t* counts;              // [8] output
};

__device__ __forceinline__ int block_coordinate(float v)
{
  return vclampi(f2i(floorf(v * 0.125f)), -kCoordinateClamp, kCoordinateClamp);
}

// the blocks [lo, hi]^3 that the eight corners of block (bx, by, bz) reach through `r`, at most `span` per axis. The
// clamp keeps lo + span an int whatever the pose holds; a block beyond it is beyond the int16 range on either side of it.
__device__ __forceinline__ void block_box(const float* r, int bx, int by, int bz, int span, int lo[3], int hi[3])
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
  hi[0] = vmini(block_coordinate(most.x), lo[0] + span - 1);
  hi[1] = vmini(block_coordinate(most.y), lo[1] + span - 1);
  hi[2] = vmini(block_coordinate(most.z), lo[2] + span - 1);
}

// sample point j of n along an axis, from the voxel's centre
__device__ __forceinline__ float point_offset(int j, int n) { return (float)(2 * j + 1) / (float)(2 * n) - 0.5f; }

// (the control words are zero: a memset in front of this launch)
__global__ __launch_bounds__(256) void resample_init_kernel(ResampleParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (P.flags & VK_MERGE_CONTINUE)
  {
    // the workspace is the previous call's: the same source blocks in the same list, their boxes, what has been fused
    int still = 0;
    if (index < P.src_total) still = P.state[index] == kConsidered ? 1 : 0;
    wave_add(&P.ctl[cConsidered], still);
    wave_add(&P.ctl[cListed], still);
  }
  else
  {
    if (index < P.src_total)
    {
      P.state[index] = kNone;
      P.flag[index] = 0;
    }
    if (index < P.dst_total) P.mark[index] = kNoCandidate;
  }
  if (index == 0) rounds_begin(P.ctl, P.dst.counters);
}

// one thread per source bucket: its source blocks (mark_chain)
__global__ __launch_bounds__(256) void resample_mark_kernel(ResampleParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  const int blocks = mark_chain(P.src, P.src_total, bucket, [&](int index) {
    P.state[index] = kConsidered;
    P.flag[index] = 1;
  });
  if (!(P.flags & VK_MERGE_SKIP_UNOBSERVED)) wave_add(&P.ctl[cConsidered], blocks);   // (classify counts otherwise)
}

// SKIP_UNOBSERVED: one wave per flagged entry; the block is ignored when every voxel's weight word is 0
__global__ __launch_bounds__(kWaveThreads) void resample_classify_kernel(ResampleParams P)
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
    if (!observed)
    {
      P.state[index] = kSkipped;
      P.flag[index] = 0;
    }
    atomicAdd(&P.ctl[observed ? cConsidered : cSkipped], 1);
  }
}

// one thread per source entry, behind the scan: the considered entries in ascending order
__global__ __launch_bounds__(256) void resample_list_kernel(ResampleParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= P.src_total) return;
  const int at = P.offset[index];
  if (at >= 0 && at < P.src_total) P.list[at] = index;
}

// entry k of the list, or -1 behind its end (the same for a whole wave)
__device__ __forceinline__ int listed_entry(const ResampleParams& P, int k)
{
  if (k >= P.src_total || k >= P.ctl[cListed]) return -1;
  const int index = P.list[k];
  return index >= 0 && index < P.src_total ? index : -1;
}

// One wave per considered source block with origin o. Each block B of o's box in dst sends the sample points of its 512
// voxels, eight voxels per lane, back into src: B is a candidate of o when one of them lands in a cell of o. One vote
// per block of the box, and no further point of a block that has one.
__global__ __launch_bounds__(kWaveThreads) void resample_geometry_kernel(ResampleParams P)
{
  const int index = listed_entry(P, blockIdx.x * kWavesPerGroup + (int)(threadIdx.x >> 6));
  if (index < 0) return;
  const Entry mine = load_entry(P.src.hash_entries, (uint32_t)index);
  const int lane = lane_id();
  int lo[3], hi[3];
  block_box(P.fwd, mine.ox, mine.oy, mine.oz, P.box, lo, hi);
  const float first_x = (float)(8 * mine.ox), first_y = (float)(8 * mine.oy), first_z = (float)(8 * mine.oz);
  const float last_x = (float)(8 * mine.ox + 7), last_y = (float)(8 * mine.oy + 7), last_z = (float)(8 * mine.oz + 7);
  const int n = P.n;
  uint32_t* bits = P.bits + (size_t)index * P.words;
  uint32_t word = 0u;
#pragma unroll 1
  for (int cell = 0; cell < P.box_cells; ++cell)
  {
    const int bx = lo[0] + cell % P.box, by = lo[1] + (cell / P.box) % P.box, bz = lo[2] + cell / (P.box * P.box);
    if (bx <= hi[0] && by <= hi[1] && bz <= hi[2] && in_int16(bx, by, bz))                  // (the same for the whole wave)
    {
      const float cx = (float)(8 * bx + (lane & 7)) + 0.5f, cy = (float)(8 * by + (lane >> 3)) + 0.5f;
      bool hit = false;
#pragma unroll 1
      for (int z = 0; z < 8; ++z)
      {
        const float cz = (float)(8 * bz + z) + 0.5f;
#pragma unroll 1
        for (int jz = 0; jz < n; ++jz)
        {
          const float pz = cz + point_offset(jz, n);
#pragma unroll 1
          for (int jy = 0; jy < n; ++jy)
          {
            const float py = cy + point_offset(jy, n);
#pragma unroll 1
            for (int jx = 0; jx < n; ++jx)
            {
              const f3 p = apply(P.back, cx + point_offset(jx, n), py, pz);
              const float qx = floorf(p.x), qy = floorf(p.y), qz = floorf(p.z);
              hit = hit || (qx >= first_x && qx <= last_x && qy >= first_y && qy <= last_y && qz >= first_z && qz <= last_z);
            }
          }
        }
        if (__any(hit ? 1 : 0)) break;
      }
      if (__any(hit ? 1 : 0)) word |= 1u << (cell & 31);
    }
    if ((cell & 31) == 31 || cell == P.box_cells - 1)
    {
      if (lane == 0) bits[cell >> 5] = word;
      word = 0u;
    }
  }
  if (lane == 0) P.lo[index] = make_int4(lo[0], lo[1], lo[2], 0);
}

// is block (bx, by, bz) of dst a candidate of the considered source entry `index`?
__device__ __forceinline__ bool candidate_of(const ResampleParams& P, int index, int bx, int by, int bz)
{
  const int4 lo = P.lo[index];
  const int rx = bx - lo.x, ry = by - lo.y, rz = bz - lo.z;
  if (rx < 0 || rx >= P.box || ry < 0 || ry >= P.box || rz < 0 || rz >= P.box) return false;
  const int cell = rx + P.box * (ry + P.box * rz);
  return (P.bits[(size_t)index * P.words + (cell >> 5)] >> (cell & 31)) & 1u;
}

// Is source entry `index` the first of the considered source blocks that have block (bx, by, bz) as a candidate? The
// others can only be among the blocks the block's own corners reach through `back`. (Absent candidates have no entry of
// dst to be counted at: each is counted by this one source block.)
__device__ __forceinline__ bool first_owner(const ResampleParams& P, int index, int bx, int by, int bz)
{
  int lo[3], hi[3];
  block_box(P.back, bx, by, bz, P.back_box, lo, hi);
  for (int oz = lo[2]; oz <= hi[2]; ++oz)
    for (int oy = lo[1]; oy <= hi[1]; ++oy)
      for (int ox = lo[0]; ox <= hi[0]; ++ox)
      {
        if (!in_int16(ox, oy, oz)) continue;
        int slot;
        Entry main_entry;
        const int other = find_block(P.src, P.src_total, ox, oy, oz, slot, main_entry);
        if (other < 0 || other >= index || P.state[other] != kConsidered) continue;
        if (candidate_of(P, other, bx, by, bz)) return false;
      }
  return true;
}

// One wave per considered source entry, the lanes striding over the blocks of its box. A lane walks the chain of its
// candidate's bucket in dst. A candidate that is there is marked at its entry, once (the compare-and-swap decides who
// counts it; a mark of an earlier call stays). POST: one that is absent asks for a slot (request_block).
template <bool POST>
__global__ __launch_bounds__(kWaveThreads) void resample_request_kernel(ResampleParams P)
{
  if (POST && P.ctl[cStop]) return;                   // the rounds are over: this one changes nothing
  const int index = listed_entry(P, blockIdx.x * kWavesPerGroup + (int)(threadIdx.x >> 6));
  if (index < 0) return;
  int marked = 0, posted = 0, absent = 0;
  const int4 lo = P.lo[index];
  const uint32_t* bits = P.bits + (size_t)index * P.words;
  for (int cell = lane_id(); cell < P.box_cells; cell += kWave)
  {
    if (!((bits[cell >> 5] >> (cell & 31)) & 1u)) continue;
    const int bx = lo.x + cell % P.box, by = lo.y + (cell / P.box) % P.box, bz = lo.z + cell / (P.box * P.box);
    int slot;
    Entry main_entry;
    const int at = find_block(P.dst, P.dst_total, bx, by, bz, slot, main_entry);
    if (at >= 0)
    {
      if (P.mark[at] == kNoCandidate) marked += atomicCAS(&P.mark[at], (int32_t)kNoCandidate, (int32_t)kCandidate) == kNoCandidate ? 1 : 0;
    }
    else if (POST)
    {
      request_block(P.dst, bx, by, bz, main_entry);
      ++posted;
    }
    else absent += first_owner(P, index, bx, by, bz) ? 1 : 0;
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

__global__ void resample_finish_kernel(ResampleParams P)
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

// One wave per marked dst entry, eight voxels per lane (lane = 8 y + x, one z per trip). The source blocks under the
// carried block — from the least block its eight corners reach, D per axis — go into the wave's LDS directory once
// (fill_directory_cells), so a sub-sample's eight neighbours cost eight pool reads and no table read. A lattice point
// outside the directory (no rigid pose at these voxel lengths gets there) counts as absent.
__global__ __launch_bounds__(kWaveThreads) void resample_fuse_kernel(ResampleParams P)
{
  extern __shared__ int directories[];                                  // [kWavesPerGroup][side^3]
  const int wave = (int)(threadIdx.x >> 6);
  const int at = blockIdx.x * kWavesPerGroup + wave;
  if (at >= P.dst_total) return;
  if (P.mark[at] != kCandidate) return;
  const Entry mine = load_entry(P.dst.hash_entries, (uint32_t)at);
  if (mine.data < 0 || mine.data >= P.dst_total) return;
  const int lane = lane_id();
  const int side = P.side;
  int* directory = directories + wave * side * side * side;

  // every sample point lies in the block's box, and a row of `back` rises or falls with each coordinate whatever the
  // rounding: no point's cell lies before the least of the corners' cells
  int least_x = INT32_MAX, least_y = INT32_MAX, least_z = INT32_MAX;
#pragma unroll
  for (int s = 0; s < 8; ++s)
  {
    const Lattice l = lattice_at(apply(P.back, (float)(8 * mine.ox + 8 * (s & 1)), (float)(8 * mine.oy + 8 * ((s >> 1) & 1)),
                                       (float)(8 * mine.oz + 8 * (s >> 2))));
    least_x = vmini(least_x, l.bx >> 3);
    least_y = vmini(least_y, l.by >> 3);
    least_z = vmini(least_z, l.bz >> 3);
  }
  fill_directory_cells(P.src, P.src_total, least_x, least_y, least_z, side, directory);

  const uint32_t* src_pool = reinterpret_cast<const uint32_t*>(P.src.voxels);
  uint32_t* mine_voxels = reinterpret_cast<uint32_t*>(P.dst.voxels) + (size_t)mine.data * VK_BLOCK_VOXELS * kVoxelWords;
  const float cap_d = P.cap_distance, cap_c = P.cap_color, scale = P.scale;
  const int n = P.n, points = P.points;
  const bool rescale = P.rescale != 0, shrinks = scale < 1.0f;
  const float cx = (float)(8 * mine.ox + (lane & 7)) + 0.5f, cy = (float)(8 * mine.oy + (lane >> 3)) + 0.5f;
  int sampled = 0;
#pragma unroll 1
  for (int z = 0; z < 8; ++z)
  {
    const float cz = (float)(8 * mine.oz + z) + 0.5f;
    float sum_d = 0.0f, sum_r = 0.0f, sum_g = 0.0f, sum_b = 0.0f;
    int count_d = 0, count_c = 0, least_dw = 32767, least_cw = 32767;
    int jx = 0, jy = 0, jz = 0;
#pragma unroll 1
    for (int j = 0; j < points; ++j)
    {
      const Lattice l = lattice_at(apply(P.back, cx + point_offset(jx, n), cy + point_offset(jy, n), cz + point_offset(jz, n)));
      if (++jx == n)
      {
        jx = 0;
        if (++jy == n)
        {
          jy = 0;
          ++jz;
        }
      }
      const bool far_x = l.fx != 0.0f, far_y = l.fy != 0.0f, far_z = l.fz != 0.0f;
      float distance[8], red[8], green[8], blue[8];
      bool has_d = true, has_c = true, saturated = false;
      int sub_dw = 32767, sub_cw = 32767;
#pragma unroll
      for (int s = 0; s < 8; ++s)
      {
        distance[s] = red[s] = green[s] = blue[s] = 0.0f;
        const bool used = (!(s & 1) || far_x) && (!(s & 2) || far_y) && (!(s & 4) || far_z);
        if (!used) continue;
        const int nx = l.bx + (s & 1), ny = l.by + ((s >> 1) & 1), nz = l.bz + (s >> 2);
        const int rx = (nx >> 3) - least_x, ry = (ny >> 3) - least_y, rz = (nz >> 3) - least_z;
        int slot = -1;
        if (rx >= 0 && rx < side && ry >= 0 && ry < side && rz >= 0 && rz < side) slot = directory[rx + side * (ry + side * rz)];
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
        saturated = saturated || distance[s] >= 1.0f;
        sub_dw = vmini(sub_dw, dw);
        sub_cw = vmini(sub_cw, cw);
      }
      if (has_d)
      {
        float sub = trilinear(distance, l.fx, l.fy, l.fz);
        if (rescale)                                 // (the same for the whole launch)
        {
          // a stored distance is in truncation lengths: into the destination's, and into the band the integrator writes
          if (shrinks && saturated) has_d = false;
          sub = scale * sub;
          sub = sub >= 1.0f ? 1.0f : sub;
          if (sub <= -1.0f) has_d = false;
        }
        if (has_d)
        {
          sum_d = count_d == 0 ? sub : sum_d + sub;
          ++count_d;
          least_dw = vmini(least_dw, sub_dw);
        }
      }
      if (has_c)
      {
        const float r = trilinear(red, l.fx, l.fy, l.fz), g = trilinear(green, l.fx, l.fy, l.fz), b = trilinear(blue, l.fx, l.fy, l.fz);
        sum_r = count_c == 0 ? r : sum_r + r;
        sum_g = count_c == 0 ? g : sum_g + g;
        sum_b = count_c == 0 ? b : sum_b + b;
        ++count_c;
        least_cw = vmini(least_cw, sub_cw);
      }
    }
    // a voxel's sample: the mean of its sub-samples where more than half of them exist
    const bool has_d = 2 * count_d > points, has_c = 2 * count_c > points;
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
        const float sample = sum_d / (float)count_d;
        const float wd = (float)dw, ws = (float)least_dw, sum = wd + ws;
        const float mean = (wd * __uint_as_float(out[0]) + ws * sample) / sum;
        out[0] = dw == 0 ? __float_as_uint(sample) : __float_as_uint(mean);
        dw = (int16_t)fminf(cap_d, sum);
        ++sampled;
      }
      if (has_c)
      {
        const float among = (float)count_c;
        const float samples[3] = {sum_r / among, sum_g / among, sum_b / among};
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

// blocks per axis that a block of 8 voxels reaches at `ratio` voxels of the other lattice per voxel: its diagonal
inline int box_blocks(float ratio)
{
  const int span = (int)(ratio * kDiagonal) + 2;
  return span < kMostBox ? span : kMostBox;
}

// blocks per axis under the lattice points of one carried block's sample points (DESIGN.md §22 has the proof)
inline int directory_blocks(float ratio)
{
  const int span = (int)(ratio * kDiagonal + 0.125f) + 2;
  return span < kMostDirectory ? span : kMostDirectory;
}

inline bool ratio_ok(float r) { return r >= 0.25f && r <= 4.0f; }     // (false for a NaN)

struct Layout
{
  size_t state, flag, offset, list, lo, bits, mark, ctl, scan, bytes;
};

inline Layout layout_of(size_t src_total, size_t dst_total, int box)
{
  const size_t words = ((size_t)box * box * box + 31) / 32;
  Layout l;
  size_t at = 0;
  l.state = at;   at += align_up(src_total);
  l.flag = at;    at += align_up(src_total * 4);
  l.offset = at;  at += align_up(src_total * 4);
  l.list = at;    at += align_up(src_total * 4);
  l.lo = at;      at += align_up(src_total * sizeof(int4));
  l.bits = at;    at += align_up(src_total * words * 4);
  l.mark = at;    at += align_up(dst_total * 4);
  l.ctl = at;     at += align_up(cWords * 4);
  l.scan = at;    at += align_up(vk_compact_workspace_bytes((int32_t)src_total));
  l.bytes = at;
  return l;
}

}  // namespace

extern "C" {

size_t vk_volume_merge_resampled_workspace_bytes(int32_t src_main, int32_t src_excess, int32_t dst_main, int32_t dst_excess,
    int32_t box_blocks_per_axis)
{
  if (src_main <= 0 || src_excess < 0 || dst_main <= 0 || dst_excess < 0) return 0;
  if (box_blocks_per_axis < 2 || box_blocks_per_axis > kMostBox) return 0;
  const size_t src_total = (size_t)src_main + (size_t)src_excess, dst_total = (size_t)dst_main + (size_t)dst_excess;
  if (src_total > (size_t)INT32_MAX || dst_total > (size_t)INT32_MAX) return 0;
  return layout_of(src_total, dst_total, box_blocks_per_axis).bytes;
}

int vk_volume_merge_resampled(const vk_volume* dst, const vk_volume* src, const vk_merge_resample_params* p, int32_t* counts_dev,
    void* workspace, void* stream)
{
  VK_REQUIRE(dst && src && p && counts_dev && workspace);
  const vk_merge_params& m = p->merge;
  VK_REQUIRE(volume_ok(dst) && volume_ok(src) && dst->voxels != src->voxels && merge_params_ok(m));
  VK_REQUIRE(p->supersample >= 1 && p->supersample <= 4 && p->reserved == 0);
  const float r_fwd = src->voxel_length / dst->voxel_length, r_back = dst->voxel_length / src->voxel_length;
  const float scale = src->truncation_length / dst->truncation_length;
  VK_REQUIRE(ratio_ok(r_fwd) && ratio_ok(r_back) && isfinite(scale) && scale > 0.0f);
  ResampleParams P;
  VK_REQUIRE(voxel_rows(p->pose.m, dst->voxel_length, P.fwd) && voxel_rows(p->pose.inv, src->voxel_length, P.back));
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 3; ++j)
    {
      P.fwd[4 * a + j] = P.fwd[4 * a + j] * r_fwd;
      P.back[4 * a + j] = P.back[4 * a + j] * r_back;
    }
  hipStream_t s = vk_s(stream);
  P.dst = *dst;
  P.src = *src;
  P.flags = m.flags;
  P.cap_distance = m.max_distance_weight;
  P.cap_color = m.max_color_weight;
  P.dst_total = dst->main_block_count + dst->excess_block_count;
  P.src_total = src->main_block_count + src->excess_block_count;
  P.scale = scale;
  P.rescale = scale != 1.0f ? 1 : 0;
  P.n = p->supersample;
  P.points = P.n * P.n * P.n;
  P.box = box_blocks(r_fwd);
  P.box_cells = P.box * P.box * P.box;
  P.words = (P.box_cells + 31) / 32;
  P.back_box = box_blocks(r_back);
  P.side = directory_blocks(r_back);
  const Layout l = layout_of((size_t)P.src_total, (size_t)P.dst_total, P.box);
  char* base = static_cast<char*>(workspace);
  P.state = reinterpret_cast<uint8_t*>(base + l.state);
  P.flag = reinterpret_cast<int32_t*>(base + l.flag);
  P.offset = reinterpret_cast<int32_t*>(base + l.offset);
  P.list = reinterpret_cast<int32_t*>(base + l.list);
  P.lo = reinterpret_cast<int4*>(base + l.lo);
  P.bits = reinterpret_cast<uint32_t*>(base + l.bits);
  P.mark = reinterpret_cast<int32_t*>(base + l.mark);
  P.ctl = reinterpret_cast<int32_t*>(base + l.ctl);
  P.counts = counts_dev;

  const int most = P.src_total > P.dst_total ? P.src_total : P.dst_total;
  const int bucket_groups = (src->main_block_count + 255) / 256, init_groups = (most + 255) / 256;
  const int src_entry_groups = (P.src_total + 255) / 256;
  const int src_wave_groups = (P.src_total + kWavesPerGroup - 1) / kWavesPerGroup;
  const int dst_wave_groups = (P.dst_total + kWavesPerGroup - 1) / kWavesPerGroup;
  const size_t directory_bytes = (size_t)kWavesPerGroup * P.side * P.side * P.side * sizeof(int);
  VK_CHECK(hipMemsetAsync(P.ctl, 0, cWords * sizeof(int32_t), s));
  hipLaunchKernelGGL(resample_init_kernel, dim3(init_groups), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  if (!(m.flags & VK_MERGE_CONTINUE))
  {
    hipLaunchKernelGGL(resample_mark_kernel, dim3(bucket_groups), dim3(256), 0, s, P);
    VK_LAUNCH_CHECK();
    if (m.flags & VK_MERGE_SKIP_UNOBSERVED)
    {
      hipLaunchKernelGGL(resample_classify_kernel, dim3(src_wave_groups), dim3(kWaveThreads), 0, s, P);
      VK_LAUNCH_CHECK();
    }
    const int code = vk_compact_offsets(P.flag, P.src_total, P.offset, &P.ctl[cListed], base + l.scan, stream);
    if (code != VK_OK) return code;
    hipLaunchKernelGGL(resample_list_kernel, dim3(src_entry_groups), dim3(256), 0, s, P);
    VK_LAUNCH_CHECK();
    hipLaunchKernelGGL(resample_geometry_kernel, dim3(src_wave_groups), dim3(kWaveThreads), 0, s, P);
    VK_LAUNCH_CHECK();
  }
  const int code = run_rounds(dst, m.max_rounds, P.ctl, stream,
      [&] { hipLaunchKernelGGL(resample_request_kernel<true>, dim3(src_wave_groups), dim3(kWaveThreads), 0, s, P); });
  if (code != VK_OK) return code;
  hipLaunchKernelGGL(resample_request_kernel<false>, dim3(src_wave_groups), dim3(kWaveThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(resample_finish_kernel, dim3(1), dim3(1), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(resample_fuse_kernel, dim3(dst_wave_groups), dim3(kWaveThreads), directory_bytes, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // extern "C"
