// vk_color_rays.hip — fuse a colour per range ray into a voxel-hashed volume, for gfx950 (no upstream counterpart: the
// reference colours only from the pixels of one pinhole image, which every voxel of a visible block finds by projecting into
// it; ref: src/color_integrator.cu:121 for the test that a voxel is near the surface, src/color_integrator.cu:125-129 for the
// running average and its cap. The definition is in include/vk.h at vk_volume_color_rays; tests/color_rays_reference.py states
// it on the CPU and the device is held to it bit for bit).
//
// Shape: everything is enqueued on the caller's stream and nothing is read back. A coloured ray walks the cells between
// r - b and r + b with vk_volume_integrate_rays' traversal, the block of the previous cell and its slot kept in registers
// (Held), and adds q_k = rintf(c_k * 1024) to the three sums of every voxel it visits in a present block and 1 to its count:
// two no-return 64-bit integer atomics, R | G << 32 and B | N << 32. A call brings at most 2^21 rays and c_k <= 1, so a sum
// is at most 2^31 and N at most 2^21: no field carries into the one above it. Integer sums commute: the sums, and the float32
// mean the fold makes of them, do not depend on ray order or timing. No float atomic touches a voxel or an accumulator.
// The band is short, so the passes are vk_volume_integrate_rays', not vk_volume_carve_rays' pool-sized memset (16 bytes per
// pool voxel here):
//   mark      one lane per ray: a byte per pool slot a coloured ray visits, a plain store of a value every writer agrees on
//   zero      one wave per marked slot zeroes its 512 x 16 bytes of accumulator
//   add       one lane per ray: the walk and the two atomics per visit; the four ray counts and the visits lost
//   fold      one wave per marked slot, eight voxels per lane: a voxel with a count that is near the surface continues its
//             colour's running average; only the colour and the colour weight are written
//   finish    the eight counts
// The call allocates nothing and leaves the table, the free list, the visible list and every counter alone.
// Every loop is bounded: the walk by its guard G (390 at most), a chain walk by the table size. No workgroup waits on
// another, and there is no LDS.
#include "vk_range_rays.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;
constexpr int kMaxCount = 1 << 21;            // N < 2^22 and a sum <= 2^31: the four fields of the two words never meet
constexpr float kMaxBand = 64.0f;             // in voxels: tb - ta <= 128, so G <= 390
constexpr float kScale = 1024.0f;             // a visit adds rintf(c * 2^10)
constexpr int kFoldSlots = 8;                 // pool slots per fold workgroup, which is one wave: one add per count and workgroup
static_assert(kFoldSlots == 8, "a workgroup reads its slots' marks as one 64-bit word");

enum { kColoured = 0, kNoColour = 1, kUnmeasured = 2, kBad = 3 };
enum { cColoured = 0, cNoColour, cNoMeasurement, cInvalid, cBlocks, cVoxels, cNotNear, cLost, cWords = 8 };

struct ColorParams : RangeRays
{
  int one_observation;
  float band, cap;
  const float* colors;          // [3 * count]
  // workspace
  unsigned long long* sums;     // [2 * 512 * total]  per pool voxel: R | G << 32, B | N << 32
  uint8_t* marks;               // [total]            1 for a pool slot a coloured ray visits
  int32_t* ctl;                 // [cWords]
  int32_t* counts;              // [8] output
};

// ray i as the call carries it, what it is by the first rule that applies, and the ends of its walk
struct ColorRay
{
  RangeRay ray;
  int what;
  float ta, tb;
  int q0, q1, q2;               // rintf(c_k * 1024) of a coloured ray
};

__device__ __forceinline__ ColorRay load_color_ray(const ColorParams& P, size_t i)
{
  ColorRay out;
  out.ray = load_range_ray(P, i);
  const float c0 = P.colors[3 * i], c1 = P.colors[3 * i + 1], c2 = P.colors[3 * i + 2];
  const bool has_colour = 0.0f <= c0 && c0 <= 1.0f && 0.0f <= c1 && c1 <= 1.0f && 0.0f <= c2 && c2 <= 1.0f;      // false for a NaN
  out.what = out.ray.kind == kInvalid ? kBad : (out.ray.kind == kNoMeasurement ? kUnmeasured : (has_colour ? kColoured : kNoColour));
  const float b = P.voxel_units ? P.band : P.band / P.v.voxel_length;
  out.ta = fmaxf(out.ray.r - b, 0.0f);
  out.tb = out.ray.r + b;
  out.q0 = has_colour ? (int)rintf(c0 * kScale) : 0;
  out.q1 = has_colour ? (int)rintf(c1 * kScale) : 0;
  out.q2 = has_colour ? (int)rintf(c2 * kScale) : 0;
  return out;
}

// One lane per ray: the slots of the blocks a coloured ray visits. Every writer of a byte writes the same value, so the
// plain store is idempotent. (The marks and the control words are zero: one memset in front of this launch.)
__global__ __launch_bounds__(kThreads) void color_mark_kernel(ColorParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)P.count) return;
  const ColorRay c = load_color_ray(P, i);
  if (c.what != kColoured) return;
  Held held;
  walk(c.ray, c.ta, c.tb, [&](int cx, int cy, int cz, float) {
    if (!held.move_to(P.v, P.total, cx >> 3, cy >> 3, cz >> 3) || held.slot < 0) return;
    if (!P.marks[held.slot]) P.marks[held.slot] = 1;
  });
}

// One wave per pool slot: a marked slot's sums and counts start from 0 (512 x 16 bytes, 16-byte stores)
__global__ __launch_bounds__(kThreads) void color_zero_kernel(ColorParams P)
{
  const int slot = blockIdx.x * (kThreads / kWave) + (int)(threadIdx.x >> 6);
  if (slot >= P.total) return;
  if (!P.marks[slot]) return;
  const int lane = lane_id();
  uint4* sums = reinterpret_cast<uint4*>(P.sums + (size_t)slot * VK_BLOCK_VOXELS * 2);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int t = 0; t < VK_BLOCK_VOXELS / kWave; ++t) sums[t * kWave + lane] = zero;
}

// One lane per ray: every visited cell of a present block adds the ray's colour to its voxel's sums and 1 to its count.
__global__ __launch_bounds__(kThreads) void color_add_kernel(ColorParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  int what = -1, lost = 0;
  if (i < (size_t)P.count)
  {
    const ColorRay c = load_color_ray(P, i);
    what = c.what;
    if (what == kColoured)
    {
      const unsigned long long low = (unsigned long long)(uint32_t)c.q0 | (unsigned long long)(uint32_t)c.q1 << 32;
      const unsigned long long high = (unsigned long long)(uint32_t)c.q2 | 1ull << 32;
      Held held;
      walk(c.ray, c.ta, c.tb, [&](int cx, int cy, int cz, float) {
        held.move_to(P.v, P.total, cx >> 3, cy >> 3, cz >> 3);
        if (!held.inside) return;
        if (held.slot < 0) { ++lost;  return; }
        const size_t voxel = (size_t)held.slot * VK_BLOCK_VOXELS + (size_t)((cz & 7) * 64 + (cy & 7) * 8 + (cx & 7));
        atomicAdd(P.sums + 2 * voxel, low);
        atomicAdd(P.sums + 2 * voxel + 1, high);
      });
    }
  }
  wave_add(&P.ctl[cColoured], what == kColoured ? 1 : 0);
  wave_add(&P.ctl[cNoColour], what == kNoColour ? 1 : 0);
  wave_add(&P.ctl[cNoMeasurement], what == kUnmeasured ? 1 : 0);
  wave_add(&P.ctl[cInvalid], what == kBad ? 1 : 0);
  wave_add(&P.ctl[cLost], lost);
}

// One wave per workgroup and kFoldSlots pool slots per wave, eight voxels per lane. A voxel with a count whose stored distance
// says it is near the surface (color_integrator.cu:121) continues its colour's running average as vk_merge.hip's fuse pass
// continues it with a source voxel of colour m and weight ws, capped as the reference caps it (color_integrator.cu:125-129);
// the distance and its weight keep their bytes, every other voxel keeps all of them. The three counts are added once per
// workgroup, behind its slots.
__global__ __launch_bounds__(kWave) void color_fold_kernel(ColorParams P)
{
  const int lane = lane_id();
  int updated = 0, refused = 0, blocks = 0;
  // the marks of the workgroup's eight slots in one load: the byte array is padded to a multiple of 256 and zeroed to its end
  const size_t first = (size_t)blockIdx.x * kFoldSlots;
  const unsigned long long marks = *reinterpret_cast<const unsigned long long*>(P.marks + first);
  if (marks == 0ull) return;
  for (int k = 0; k < kFoldSlots; ++k)
  {
    const size_t slot = first + (size_t)k;
    if (slot >= (size_t)P.total) break;
    if (!((marks >> (8 * k)) & 0xffull)) continue;
    const uint4* sums = reinterpret_cast<const uint4*>(P.sums + slot * VK_BLOCK_VOXELS * 2);
    uint32_t* block = reinterpret_cast<uint32_t*>(P.v.voxels) + slot * VK_BLOCK_VOXELS * kVoxelWords;
    constexpr int kTrips = VK_BLOCK_VOXELS / kWave;
    // every load of the lane's eight voxels is issued before the first is used
    uint4 word[kTrips];
    vu4 head[kTrips];
    uint32_t weights[kTrips];
#pragma unroll
    for (int t = 0; t < kTrips; ++t)
    {
      const int voxel = t * kWave + lane;
      word[t] = sums[voxel];
      head[t] = *reinterpret_cast<const vu4*>(block + (size_t)voxel * kVoxelWords);
      weights[t] = block[(size_t)voxel * kVoxelWords + 4];
    }
    int here = 0;
#pragma unroll
    for (int t = 0; t < kTrips; ++t)
    {
      const uint32_t N = word[t].w;
      if (N == 0u) continue;
      if (!(fabsf(__uint_as_float(head[t].x)) < 1.0f)) { ++refused;  continue; }       // (a NaN is not near)
      const float n = (float)N;
      const float m0 = ((float)word[t].x / n) * 0x1p-10f, m1 = ((float)word[t].y / n) * 0x1p-10f, m2 = ((float)word[t].z / n) * 0x1p-10f;
      const float ws = P.one_observation ? 1.0f : n;
      const int16_t c_weight = (int16_t)(weights[t] >> 16);
      const float wc = (float)c_weight;
      const float sum = wc + ws;
      uint32_t* words = block + (size_t)(t * kWave + lane) * kVoxelWords;
      words[1] = __float_as_uint(c_weight == 0 ? m0 : (wc * __uint_as_float(head[t].y) + ws * m0) / sum);
      words[2] = __float_as_uint(c_weight == 0 ? m1 : (wc * __uint_as_float(head[t].z) + ws * m1) / sum);
      words[3] = __float_as_uint(c_weight == 0 ? m2 : (wc * __uint_as_float(head[t].w) + ws * m2) / sum);
      reinterpret_cast<uint16_t*>(words + 4)[1] = (uint16_t)(int16_t)fminf(P.cap, sum);
      ++here;
    }
    updated += here;
    blocks += __any(here) != 0 ? 1 : 0;
  }
  wave_add(&P.ctl[cVoxels], updated);
  wave_add(&P.ctl[cNotNear], refused);
  if (lane == 0 && blocks) atomicAdd(&P.ctl[cBlocks], blocks);
}

__global__ void color_finish_kernel(ColorParams P)
{
  const int32_t* ctl = P.ctl;
  P.counts[0] = ctl[cColoured];
  P.counts[1] = ctl[cNoColour];
  P.counts[2] = ctl[cNoMeasurement];
  P.counts[3] = ctl[cInvalid];
  P.counts[4] = ctl[cBlocks];
  P.counts[5] = ctl[cVoxels];
  P.counts[6] = ctl[cNotNear];
  P.counts[7] = ctl[cLost];
}

// vk_volume_color_rays_time_next: the events the next call of this host thread records between its passes
constexpr int kPassEvents = 5;
thread_local hipEvent_t g_pass_events[kPassEvents] = {};
thread_local bool g_pass_armed = false;

}  // namespace

extern "C" {

int vk_volume_color_rays_time_next(void* const* events, int32_t count)
{
  VK_REQUIRE((events == nullptr && count == 0) || (events != nullptr && count == kPassEvents));
  for (int k = 0; k < kPassEvents; ++k)
  {
    VK_REQUIRE(events == nullptr || events[k] != nullptr);
    g_pass_events[k] = events ? static_cast<hipEvent_t>(events[k]) : nullptr;
  }
  g_pass_armed = events != nullptr;
  return VK_OK;
}

size_t vk_volume_color_rays_workspace_bytes(int32_t main, int32_t excess)
{
  if (main <= 0 || excess < 0) return 0;
  const size_t total = (size_t)main + (size_t)excess;
  if (total > (size_t)INT32_MAX) return 0;
  return align_up(total * VK_BLOCK_VOXELS * 16) + align_up(total) + align_up(cWords * 4);
}

int vk_volume_color_rays(const vk_volume* v, const float* rays, const float* ranges, const float* colors, int32_t count,
    const vk_transform* pose_dev, const vk_color_rays_params* p, int32_t* counts_dev, void* workspace, void* stream)
{
  // the events are used up by this call, whether or not it gets as far as its launches (as vk_volume_integrate_rays_time_next's are)
  const bool timed = g_pass_armed;
  g_pass_armed = false;
  VK_REQUIRE(v && p && counts_dev);
  VK_REQUIRE(p->max_color_weight >= 1.0f && p->max_color_weight <= 32767.0f);            // (false for a NaN)
  VK_REQUIRE(__builtin_isfinite(p->band) && p->band > 0.0f);
  VK_REQUIRE(colors || count == 0);
  ColorParams P;
  VK_REQUIRE(range_rays_arguments(v, rays, ranges, count, pose_dev, p->flags, p->r_min, p->r_max, workspace,
      VK_RAYS_VOXEL_UNITS | VK_RAYS_ONE_OBSERVATION, kMaxCount, true, true, P) == VK_OK);
  VK_REQUIRE((P.voxel_units ? p->band : p->band / v->voxel_length) <= kMaxBand);
  if (count == 0) return VK_OK;
  hipStream_t s = vk_s(stream);
  P.one_observation = (p->flags & VK_RAYS_ONE_OBSERVATION) ? 1 : 0;
  P.band = p->band;
  P.cap = p->max_color_weight;
  P.colors = colors;
  const size_t total = (size_t)P.total;
  char* at = static_cast<char*>(workspace);
  P.sums = reinterpret_cast<unsigned long long*>(at);   at += align_up(total * VK_BLOCK_VOXELS * 16);
  P.marks = reinterpret_cast<uint8_t*>(at);             at += align_up(total);
  P.ctl = reinterpret_cast<int32_t*>(at);
  P.counts = counts_dev;

  const unsigned ray_groups = (unsigned)(((size_t)count + kThreads - 1) / kThreads);
  const unsigned wave_groups = (unsigned)((total + kThreads / kWave - 1) / (kThreads / kWave));
  const unsigned fold_groups = (unsigned)((total + kFoldSlots - 1) / kFoldSlots);
  int pass = 0;
  const auto pass_done = [&]() { return timed ? hipEventRecord(g_pass_events[pass++], s) : hipSuccess; };
  VK_CHECK(pass_done());
  VK_CHECK(hipMemsetAsync(P.marks, 0, align_up(total) + cWords * sizeof(int32_t), s));   // the marks, and the control words behind them
  hipLaunchKernelGGL(color_mark_kernel, dim3(ray_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  hipLaunchKernelGGL(color_zero_kernel, dim3(wave_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  hipLaunchKernelGGL(color_add_kernel, dim3(ray_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  hipLaunchKernelGGL(color_fold_kernel, dim3(fold_groups), dim3(kWave), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(color_finish_kernel, dim3(1), dim3(1), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  return VK_OK;
}

}  // extern "C"
