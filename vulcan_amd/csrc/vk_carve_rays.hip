// vk_carve_rays.hip — carve free space along range rays in a voxel-hashed volume, for gfx950 (no upstream counterpart: the
// reference integrator writes min(1, d / truncation) = 1 into every voxel of a visible block in front of the surface of one
// pinhole depth image, ref: src/depth_integrator.cu:54-74; vk_volume_integrate_rays fuses only the band around a range ray's
// measurement and this call does the rest of the ray. The definition is in include/vk.h at vk_volume_carve_rays;
// tests/carve_rays_reference.py states it on the CPU and the device is held to it bit for bit).
//
// Shape: everything is enqueued on the caller's stream and nothing is read back. A ray walks the blocks it crosses between
// t_from and the start of its band, one chain walk per block; almost all of them are absent and are passed over. In a block
// that exists the ray walks its cells with vk_volume_integrate_rays' traversal and adds 1 to the count N of every voxel it
// leaves before the band begins: a no-return 32-bit integer atomic. Every carve observes the distance 1, so a count is all
// there is to keep; counts commute, and no float atomic touches a voxel or an accumulator. The rays walk once: there is no
// mark pass in front that would say which slots to zero, so one memset zeroes all of N, 4 bytes per pool voxel.
//   memset    N, the byte per pool slot and the control words: one hipMemsetAsync, its size follows the pool, not the rays
//   add       one lane per ray: the block walk, the cell walk in a present block, the carves; the five ray counts
//   fold      one wave per eight pool slots: a touched slot's voxels with a count continue their running average with 1
//   finish    the eight counts
// The call allocates nothing and leaves the table, the free list, the visible list and every counter alone.
// Every loop is bounded: the block walk by max_blocks, a cell walk by its guard (48 at most), a chain walk by the table size.
// No workgroup waits on another, and there is no LDS.
#include "vk_range_rays.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;
constexpr int kMaxCount = 1 << 22;
constexpr int kMaxBlocks = 4096;
constexpr int kFoldSlots = 8;                 // pool slots per fold workgroup, which is one wave: one add per count and workgroup
static_assert(kFoldSlots == 8, "a workgroup reads its slots' bytes as one 64-bit word");

enum { cCarved = 0, cNothing, cNoMeasurement, cInvalid, cCut, cBlocks, cVoxels, cCarves, cWords = 8 };

struct CarveParams : RangeRays
{
  int one_observation;
  int max_blocks;
  float t_from, cap;
  // workspace
  uint32_t* visits;             // [512 * total]  N per pool voxel
  uint8_t* touched;             // [total]        1 for a pool slot that took a carve
  int32_t* ctl;                 // [cWords]
  int32_t* counts;              // [8] output
};

// One lane per ray. (N, the touched bytes and the control words are zero: one memset in front of this launch.)
__global__ __launch_bounds__(kThreads) void carve_add_kernel(CarveParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  int what = -1, cut = 0, carves = 0;
  if (i < (size_t)P.count)
  {
    const RangeRay ray = load_range_ray(P, i);
    const float tr = P.v.truncation_length / P.v.voxel_length;
    const float t0 = P.voxel_units ? P.t_from : P.t_from / P.v.voxel_length;
    const float te = ray.r - tr;
    what = ray.kind == kInvalid ? cInvalid : (ray.kind == kNoMeasurement ? cNoMeasurement : (t0 < te ? cCarved : cNothing));
    if (what == cCarved)
    {
      const float px = ray.o.x + t0 * ray.n.x, py = ray.o.y + t0 * ray.n.y, pz = ray.o.z + t0 * ray.n.z;
      int bx = cell_of(px) >> 3, by = cell_of(py) >> 3, bz = cell_of(pz) >> 3;
      int sx, sy, sz;
      float mx, my, mz, dx, dy, dz;
      axis_setup<8>(t0, px, ray.n.x, bx, sx, mx, dx);
      axis_setup<8>(t0, py, ray.n.y, by, sy, my, dy);
      axis_setup<8>(t0, pz, ray.n.z, bz, sz, mz, dz);
      float t_in = t0;
      cut = 1;
      for (int turn = 0; turn < P.max_blocks; ++turn)
      {
        float least;
        const int axis = least_axis(mx, my, mz, least);       // of the block faces
        const float t_out = fminf(least, te);
        int slot = -1;
        Entry main_entry;
        if (in_int16(bx, by, bz)) find_block(P.v, P.total, bx, by, bz, slot, main_entry);
        if (slot >= 0)
        {
          uint32_t* visits = P.visits + (size_t)slot * VK_BLOCK_VOXELS;
          int here = 0;
          walk(ray, t_in, t_out, [&](int cx, int cy, int cz, float leaves_at) {
            // a cell of another block is that block's to carve; the cell the band begins in is the band walk's
            if ((cx >> 3) != bx || (cy >> 3) != by || (cz >> 3) != bz || !(leaves_at <= te)) return;
            atomicAdd(visits + ((cz & 7) * 64 + (cy & 7) * 8 + (cx & 7)), 1u);
            ++here;
          });
          // every writer of the byte writes the same value: the plain store is idempotent
          if (here) P.touched[slot] = 1;
          carves += here;
        }
        if (!(least < te)) { cut = 0;  break; }
        if (axis == 0) { bx += sx;  mx = mx + dx; }
        else if (axis == 1) { by += sy;  my = my + dy; }
        else { bz += sz;  mz = mz + dz; }
        t_in = least;
      }
    }
  }
  wave_add(&P.ctl[cCarved], what == cCarved ? 1 : 0);
  wave_add(&P.ctl[cNothing], what == cNothing ? 1 : 0);
  wave_add(&P.ctl[cNoMeasurement], what == cNoMeasurement ? 1 : 0);
  wave_add(&P.ctl[cInvalid], what == cInvalid ? 1 : 0);
  wave_add(&P.ctl[cCut], cut);
  wave_add(&P.ctl[cCarves], carves);
}

// One wave per workgroup and kFoldSlots pool slots per wave, eight voxels per lane. A voxel with a count continues its
// running average as rays_fold_kernel continues it, with a mean of exactly 1 (depth_integrator.cu:55-59); the colour fields
// and the colour weight keep their bytes, a voxel without a count keeps all of them. The two counts are added once per
// workgroup, behind its slots.
__global__ __launch_bounds__(kWave) void carve_fold_kernel(CarveParams P)
{
  const int lane = lane_id();
  int updated = 0, blocks = 0;
  // the bytes of the workgroup's eight slots in one load: the byte array is padded to a multiple of 256 and zeroed to its end
  const size_t first = (size_t)blockIdx.x * kFoldSlots;
  const unsigned long long touched = *reinterpret_cast<const unsigned long long*>(P.touched + first);
  if (touched == 0ull) return;
  for (int k = 0; k < kFoldSlots; ++k)
  {
    const size_t slot = first + (size_t)k;
    if (slot >= (size_t)P.total) break;
    if (!((touched >> (8 * k)) & 0xffull)) continue;
    const uint32_t* visits = P.visits + (size_t)slot * VK_BLOCK_VOXELS;
    uint32_t* block = reinterpret_cast<uint32_t*>(P.v.voxels) + (size_t)slot * VK_BLOCK_VOXELS * kVoxelWords;
    constexpr int kTrips = VK_BLOCK_VOXELS / kWave;
    // every load of the lane's eight voxels is issued before the first is used
    uint32_t count[kTrips], distance[kTrips], weights[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; ++t)
    {
      const int voxel = t * kWave + lane;
      count[t] = visits[voxel];
      distance[t] = block[(size_t)voxel * kVoxelWords];
      weights[t] = block[(size_t)voxel * kVoxelWords + 4];
    }
    int here = 0;
#pragma unroll
    for (int t = 0; t < kTrips; ++t)
    {
      const uint32_t N = count[t];
      if (N == 0u) continue;
      const float ws = P.one_observation ? 1.0f : (float)N;
      const int16_t d_weight = (int16_t)(weights[t] & 0xffffu);
      const float wd = (float)d_weight;
      const float sum = wd + ws;
      const float mean = (wd * __uint_as_float(distance[t]) + ws) / sum;
      uint32_t* words = block + (size_t)(t * kWave + lane) * kVoxelWords;
      words[0] = d_weight == 0 ? __float_as_uint(1.0f) : __float_as_uint(mean);
      words[4] = (weights[t] & 0xffff0000u) | (uint32_t)(uint16_t)(int16_t)fminf(P.cap, sum);
      ++here;
    }
    updated += here;
    blocks += __any(here) != 0 ? 1 : 0;
  }
  wave_add(&P.ctl[cVoxels], updated);
  if (lane == 0 && blocks) atomicAdd(&P.ctl[cBlocks], blocks);
}

__global__ void carve_finish_kernel(CarveParams P)
{
  const int32_t* ctl = P.ctl;
  P.counts[0] = ctl[cCarved];
  P.counts[1] = ctl[cNothing];
  P.counts[2] = ctl[cNoMeasurement];
  P.counts[3] = ctl[cInvalid];
  P.counts[4] = ctl[cCut];
  P.counts[5] = ctl[cBlocks];
  P.counts[6] = ctl[cVoxels];
  P.counts[7] = ctl[cCarves];
}

}  // namespace

extern "C" {

size_t vk_volume_carve_rays_workspace_bytes(int32_t main, int32_t excess)
{
  if (main <= 0 || excess < 0) return 0;
  const size_t total = (size_t)main + (size_t)excess;
  if (total > (size_t)INT32_MAX) return 0;
  return align_up(total * VK_BLOCK_VOXELS * 4) + align_up(total) + align_up(cWords * 4);
}

int vk_volume_carve_rays(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* pose_dev,
    const vk_carve_rays_params* p, int32_t* counts_dev, void* workspace, void* stream)
{
  VK_REQUIRE(v && p && counts_dev);
  VK_REQUIRE(p->max_blocks >= 1 && p->max_blocks <= kMaxBlocks);
  VK_REQUIRE(p->max_distance_weight >= 1.0f && p->max_distance_weight <= 32767.0f);      // (false for a NaN)
  VK_REQUIRE(__builtin_isfinite(p->t_from) && p->t_from >= 0.0f);
  CarveParams P;
  VK_REQUIRE(range_rays_arguments(v, rays, ranges, count, pose_dev, p->flags, p->r_min, p->r_max, workspace,
      VK_RAYS_VOXEL_UNITS | VK_RAYS_ONE_OBSERVATION, kMaxCount, true, true, P) == VK_OK);
  if (count == 0) return VK_OK;
  hipStream_t s = vk_s(stream);
  P.one_observation = (p->flags & VK_RAYS_ONE_OBSERVATION) ? 1 : 0;
  P.max_blocks = p->max_blocks;
  P.t_from = p->t_from;
  P.cap = p->max_distance_weight;
  const size_t total = (size_t)P.total;
  char* at = static_cast<char*>(workspace);
  P.visits = reinterpret_cast<uint32_t*>(at);           at += align_up(total * VK_BLOCK_VOXELS * 4);
  P.touched = reinterpret_cast<uint8_t*>(at);           at += align_up(total);
  P.ctl = reinterpret_cast<int32_t*>(at);
  P.counts = counts_dev;

  const unsigned ray_groups = (unsigned)(((size_t)count + kThreads - 1) / kThreads);
  const unsigned fold_groups = (unsigned)((total + kFoldSlots - 1) / kFoldSlots);
  // the counts, the touched bytes and the control words behind them
  VK_CHECK(hipMemsetAsync(workspace, 0, align_up(total * VK_BLOCK_VOXELS * 4) + align_up(total) + cWords * sizeof(int32_t), s));
  hipLaunchKernelGGL(carve_add_kernel, dim3(ray_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(carve_fold_kernel, dim3(fold_groups), dim3(kWave), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(carve_finish_kernel, dim3(1), dim3(1), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // extern "C"
