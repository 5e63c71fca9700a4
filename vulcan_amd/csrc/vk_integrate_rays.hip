// vk_integrate_rays.hip — fuse arbitrary range rays into a voxel-hashed volume, for gfx950 (no upstream counterpart: the
// reference fuses only the pixels of one pinhole depth image; ref: src/depth_integrator.cu:54-74 for the band test, the
// min(1, d / truncation) and the running average, src/volume.cu:87-301 for requesting the blocks within one truncation
// length either side of the measurement, src/volume.cu:304-368 for the handle pass. The definition is in include/vk.h at
// vk_volume_integrate_rays; tests/integrate_rays_reference.py states it on the CPU and the device is held to it bit for bit).
//
// Shape: everything is enqueued on the caller's stream and nothing is read back. It is the first scatter of the library:
// rays that share a voxel add to it in whatever order they arrive, so what they add is an integer: q = rintf(u * 2^20) to
// the voxel's sum S and 1 to its count N, with no-return integer atomics. Integer sums commute: the sums, and the one
// float32 mean the fold makes of them, do not depend on ray order or timing. No float atomic touches a voxel or an
// accumulator. A call of fewer than 2^21 rays packs both into one 64-bit word, N above bit 43 and the sum of q + 2^20
// below it (N < 2^21 and the biased sum <= N 2^21 < 2^42 cannot meet): one atomic per update. 64 bits cannot hold both for
// the 2^22 rays a call may bring (23 bits of N, 44 of the sum), so a larger call adds to a 64-bit S and a 32-bit N apart. Every pass that follows the rays is one lane per ray and walks the cells of the ray's band with the block
// of the previous cell and its slot kept in registers, so a chain is walked once per block (about eight cells), not per cell.
//   snapshot  per table entry: which pool slots hold a block before the call (the count of blocks allocated needs it)
//   rounds    max_rounds times: rays walk and post a request for every absent block (the largest key wins the bucket),
//             the existing handle pass, round end (run_rounds, vk_alloc_rounds.hpp)
//   mark      rays walk and set a byte per pool slot they visit: a plain store of a value every writer agrees on
//   zero      one wave per marked slot zeroes its 512 accumulators
//   add       rays walk and add, one atomic per update (two from 2^21 rays on); the three ray counts and the visits lost
//   fold      one wave per marked slot: the voxels with a count continue their running average with the mean
//   finish    the eight counts, VK_CTR_VISIBLE and VK_CTR_BANDED
// Every loop is bounded: the walk by its guard G, a chain walk by the table size. No workgroup waits on another.
#include "vk_alloc_rounds.hpp"
#include "vk_range_rays.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;
constexpr int kMaxCount = 1 << 22;
constexpr int kPackedCount = 1 << 21;       // below this many rays a voxel's N and biased sum share one 64-bit word
constexpr int kCountShift = 43;
constexpr int kBias = 1 << 20;

enum : uint8_t { kHeldBefore = 1, kVisited = 2 };
// the words that carry the sums, behind the ones that steer the rounds
enum { cIntegrated = cRoundWords, cNoMeasurement, cInvalid, cAllocated, cBlocks, cVoxels, cLost, cWords = 16 };
struct RaysParams : RangeRays
{
  int one_observation;
  float cap;
  // workspace
  unsigned long long* sums;     // [512 * total]  two's complement sum of q per pool voxel; PACKED: N << 43 | sum of (q + 2^20)
  uint32_t* visits;             // [512 * total]  N per pool voxel (not PACKED)
  uint8_t* marks;               // [total]        kHeldBefore | kVisited per pool slot
  int32_t* ctl;                 // [cWords]
  int32_t* counts;              // [8] output
};

// the cells of the ray's band, between ta = max(r - tr, 0) and tb = r + tr: visit(cx, cy, cz) per cell
template <class Visit>
__device__ __forceinline__ void walk(const RangeRay& ray, float tr, Visit&& visit)
{
  vk::walk(ray, fmaxf(ray.r - tr, 0.0f), ray.r + tr, [&](int cx, int cy, int cz, float) { visit(cx, cy, cz); });
}

// (the control words and the marks are zero: one memset in front of this launch)
__global__ __launch_bounds__(kThreads) void rays_snapshot_kernel(RaysParams P)
{
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index < P.total)
  {
    const int data = P.v.hash_entries[index].data;
    if (data >= 0 && data < P.total) P.marks[data] = kHeldBefore;
  }
  if (index == 0) rounds_begin(P.ctl, P.v.counters);
}

// One lane per ray. An absent block of a visited cell asks for a slot (request_block).
__global__ __launch_bounds__(kThreads) void rays_request_kernel(RaysParams P)
{
  if (P.ctl[cStop]) return;                           // the rounds are over: this one changes nothing
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  int posted = 0;
  if (i < (size_t)P.count)
  {
    const RangeRay ray = load_range_ray(P, i);
    if (ray.kind == kIntegrated)
    {
      const float tr = P.v.truncation_length / P.v.voxel_length;
      Held held;
      walk(ray, tr, [&](int cx, int cy, int cz) {
        if (!held.move_to(P.v, P.total, cx >> 3, cy >> 3, cz >> 3) || !held.inside || held.slot >= 0) return;
        request_block(P.v, held.x, held.y, held.z, held.main_entry);
        posted = 1;
      });
    }
  }
  wave_add(&P.ctl[cPosted], posted);
}

// One lane per ray: the slots of the blocks it visits. Every writer of a byte writes the same value (kHeldBefore does not
// change during the pass), so the plain store is idempotent.
__global__ __launch_bounds__(kThreads) void rays_mark_kernel(RaysParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)P.count) return;
  const RangeRay ray = load_range_ray(P, i);
  if (ray.kind != kIntegrated) return;
  const float tr = P.v.truncation_length / P.v.voxel_length;
  Held held;
  walk(ray, tr, [&](int cx, int cy, int cz) {
    if (!held.move_to(P.v, P.total, cx >> 3, cy >> 3, cz >> 3) || held.slot < 0) return;
    const uint8_t mark = P.marks[held.slot];
    if (!(mark & kVisited)) P.marks[held.slot] = mark | kVisited;
  });
}

// One wave per pool slot: a visited slot's sums and counts start from 0 (16-byte stores)
template <bool PACKED>
__global__ __launch_bounds__(kThreads) void rays_zero_kernel(RaysParams P)
{
  const int slot = blockIdx.x * (kThreads / kWave) + (int)(threadIdx.x >> 6);
  if (slot >= P.total) return;
  if (!(P.marks[slot] & kVisited)) return;
  const int lane = lane_id();
  uint4* sums = reinterpret_cast<uint4*>(P.sums + (size_t)slot * VK_BLOCK_VOXELS);
  uint4* visits = reinterpret_cast<uint4*>(P.visits + (size_t)slot * VK_BLOCK_VOXELS);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int t = 0; t < 4; ++t) sums[t * kWave + lane] = zero;           // 512 x 8 bytes = 256 vectors
  if (PACKED) return;
#pragma unroll
  for (int t = 0; t < 2; ++t) visits[t * kWave + lane] = zero;         // 512 x 4 bytes = 128 vectors
}

// One lane per ray: every visited cell of a present block that passes the band test adds q to its voxel's sum and 1 to
// its count.
template <bool PACKED>
__global__ __launch_bounds__(kThreads) void rays_add_kernel(RaysParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  int kind = -1, lost = 0;
  if (i < (size_t)P.count)
  {
    const RangeRay ray = load_range_ray(P, i);
    kind = ray.kind;
    if (kind == kIntegrated)
    {
      const float tr = P.v.truncation_length / P.v.voxel_length;
      Held held;
      walk(ray, tr, [&](int cx, int cy, int cz) {
        held.move_to(P.v, P.total, cx >> 3, cy >> 3, cz >> 3);
        if (!held.inside) return;
        if (held.slot < 0) { ++lost;  return; }
        const float ex = (float)cx + 0.5f, ey = (float)cy + 0.5f, ez = (float)cz + 0.5f;
        const float raw = ray.r - (((ex - ray.o.x) * ray.n.x + (ey - ray.o.y) * ray.n.y) + (ez - ray.o.z) * ray.n.z);
        if (!(raw > -tr)) return;
        const float u = fminf(1.0f, raw / tr);
        const int q = (int)rintf(u * 1048576.0f);
        const size_t voxel = (size_t)held.slot * VK_BLOCK_VOXELS + (size_t)((cz & 7) * 64 + (cy & 7) * 8 + (cx & 7));
        if (PACKED) atomicAdd(P.sums + voxel, (1ull << kCountShift) + (unsigned long long)(q + kBias));
        else
        {
          atomicAdd(P.sums + voxel, (unsigned long long)(long long)q);
          atomicAdd(P.visits + voxel, 1u);
        }
      });
    }
  }
  wave_add(&P.ctl[cIntegrated], kind == kIntegrated ? 1 : 0);
  wave_add(&P.ctl[cNoMeasurement], kind == kNoMeasurement ? 1 : 0);
  wave_add(&P.ctl[cInvalid], kind == kInvalid ? 1 : 0);
  wave_add(&P.ctl[cLost], lost);
}

// One wave per pool slot, eight voxels per lane. A voxel with a count continues its running average as vk_merge.hip's fuse
// pass does with a source voxel of distance m and weight ws (depth_integrator.cu:55-59); the colour fields and the colour
// weight keep their bytes, a voxel without a count keeps all of them.
template <bool PACKED>
__global__ __launch_bounds__(kThreads) void rays_fold_kernel(RaysParams P)
{
  const int slot = blockIdx.x * (kThreads / kWave) + (int)(threadIdx.x >> 6);
  if (slot >= P.total) return;
  const uint8_t mark = P.marks[slot];
  if (!(mark & kVisited)) return;
  const int lane = lane_id();
  const unsigned long long* sums = P.sums + (size_t)slot * VK_BLOCK_VOXELS;
  const uint32_t* visits = P.visits + (size_t)slot * VK_BLOCK_VOXELS;
  uint32_t* block = reinterpret_cast<uint32_t*>(P.v.voxels) + (size_t)slot * VK_BLOCK_VOXELS * kVoxelWords;
  constexpr int kTrips = VK_BLOCK_VOXELS / kWave;
  // every load of the lane's eight voxels is issued before the first is used
  unsigned long long word[kTrips];
  uint32_t count[kTrips], distance[kTrips], weights[kTrips];
#pragma unroll
  for (int t = 0; t < kTrips; ++t)
  {
    const int voxel = t * kWave + lane;
    word[t] = sums[voxel];
    count[t] = PACKED ? 0u : visits[voxel];
    distance[t] = block[(size_t)voxel * kVoxelWords];
    weights[t] = block[(size_t)voxel * kVoxelWords + 4];
  }
  int updated = 0;
#pragma unroll
  for (int t = 0; t < kTrips; ++t)
  {
    const uint32_t N = PACKED ? (uint32_t)(word[t] >> kCountShift) : count[t];
    if (N == 0u) continue;
    const long long S = PACKED ? (long long)(word[t] & ((1ull << kCountShift) - 1ull)) - (long long)N * kBias : (long long)word[t];
    const float m = ((float)S / (float)N) * 0x1p-20f;
    const float ws = P.one_observation ? 1.0f : (float)N;
    const int16_t d_weight = (int16_t)(weights[t] & 0xffffu);
    const float wd = (float)d_weight;
    const float sum = wd + ws;
    const float mean = (wd * __uint_as_float(distance[t]) + ws * m) / sum;
    uint32_t* words = block + (size_t)(t * kWave + lane) * kVoxelWords;
    words[0] = d_weight == 0 ? __float_as_uint(m) : __float_as_uint(mean);
    words[4] = (weights[t] & 0xffff0000u) | (uint32_t)(uint16_t)(int16_t)fminf(P.cap, sum);
    ++updated;
  }
  wave_add(&P.ctl[cVoxels], updated);
  const bool any = __any(updated) != 0;
  if (lane == 0)
  {
    if (any) atomicAdd(&P.ctl[cBlocks], 1);
    if (!(mark & kHeldBefore)) atomicAdd(&P.ctl[cAllocated], 1);
  }
}

__global__ void rays_finish_kernel(RaysParams P)
{
  const int32_t* ctl = P.ctl;
  P.counts[0] = ctl[cIntegrated];
  P.counts[1] = ctl[cNoMeasurement];
  P.counts[2] = ctl[cInvalid];
  P.counts[3] = ctl[cAllocated];
  P.counts[4] = ctl[cRounds];
  P.counts[5] = ctl[cBlocks];
  P.counts[6] = ctl[cVoxels];
  P.counts[7] = ctl[cLost];
  lists_stale(P.v.counters);
}

// vk_volume_integrate_rays_time_next: the events the next call of this host thread records between its passes
constexpr int kPassEvents = 6;
thread_local hipEvent_t g_pass_events[kPassEvents] = {};
thread_local bool g_pass_armed = false;

}  // namespace

extern "C" {

int vk_volume_integrate_rays_time_next(void* const* events, int32_t count)
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

size_t vk_volume_integrate_rays_workspace_bytes(int32_t main, int32_t excess)
{
  if (main <= 0 || excess < 0) return 0;
  const size_t total = (size_t)main + (size_t)excess;
  if (total > (size_t)INT32_MAX) return 0;
  return align_up(total * VK_BLOCK_VOXELS * 8) + align_up(total * VK_BLOCK_VOXELS * 4) + align_up(total) + align_up(cWords * 4);
}

int vk_volume_integrate_rays(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* pose_dev,
    const vk_integrate_rays_params* p, int32_t* counts_dev, void* workspace, void* stream)
{
  // the events are used up by this call, whether or not it gets as far as its launches (as vk_integrate_time_next's are)
  const bool timed = g_pass_armed;
  g_pass_armed = false;
  VK_REQUIRE(v && p && counts_dev);
  VK_REQUIRE(p->max_rounds >= 0 && p->max_rounds <= 64);
  VK_REQUIRE(p->max_distance_weight >= 1.0f && p->max_distance_weight <= 32767.0f);      // (false for a NaN)
  RaysParams P;
  VK_REQUIRE(range_rays_arguments(v, rays, ranges, count, pose_dev, p->flags, p->r_min, p->r_max, workspace,
      VK_RAYS_VOXEL_UNITS | VK_RAYS_ONE_OBSERVATION, kMaxCount, true, true, P) == VK_OK);
  if (count == 0) return VK_OK;
  hipStream_t s = vk_s(stream);
  P.one_observation = (p->flags & VK_RAYS_ONE_OBSERVATION) ? 1 : 0;
  P.cap = p->max_distance_weight;
  const size_t total = (size_t)P.total;
  char* at = static_cast<char*>(workspace);
  P.sums = reinterpret_cast<unsigned long long*>(at);   at += align_up(total * VK_BLOCK_VOXELS * 8);
  P.visits = reinterpret_cast<uint32_t*>(at);           at += align_up(total * VK_BLOCK_VOXELS * 4);
  P.marks = reinterpret_cast<uint8_t*>(at);             at += align_up(total);
  P.ctl = reinterpret_cast<int32_t*>(at);
  P.counts = counts_dev;

  const unsigned ray_groups = (unsigned)(((size_t)count + kThreads - 1) / kThreads);
  const unsigned entry_groups = (unsigned)((total + kThreads - 1) / kThreads);
  const unsigned wave_groups = (unsigned)((total + kThreads / kWave - 1) / (kThreads / kWave));
  int pass = 0;
  const auto pass_done = [&]() { return timed ? hipEventRecord(g_pass_events[pass++], s) : hipSuccess; };
  VK_CHECK(pass_done());
  VK_CHECK(hipMemsetAsync(P.marks, 0, align_up(total) + cWords * sizeof(int32_t), s));   // the marks, and the control words behind them
  hipLaunchKernelGGL(rays_snapshot_kernel, dim3(entry_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  const int code = run_rounds(v, p->max_rounds, P.ctl, stream,
      [&] { hipLaunchKernelGGL(rays_request_kernel, dim3(ray_groups), dim3(kThreads), 0, s, P); });
  if (code != VK_OK) return code;
  VK_CHECK(pass_done());
  hipLaunchKernelGGL(rays_mark_kernel, dim3(ray_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  const bool packed = count < kPackedCount;
  if (packed) hipLaunchKernelGGL(rays_zero_kernel<true>, dim3(wave_groups), dim3(kThreads), 0, s, P);
  else hipLaunchKernelGGL(rays_zero_kernel<false>, dim3(wave_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  if (packed) hipLaunchKernelGGL(rays_add_kernel<true>, dim3(ray_groups), dim3(kThreads), 0, s, P);
  else hipLaunchKernelGGL(rays_add_kernel<false>, dim3(ray_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  if (packed) hipLaunchKernelGGL(rays_fold_kernel<true>, dim3(wave_groups), dim3(kThreads), 0, s, P);
  else hipLaunchKernelGGL(rays_fold_kernel<false>, dim3(wave_groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(rays_finish_kernel, dim3(1), dim3(1), 0, s, P);
  VK_LAUNCH_CHECK();
  VK_CHECK(pass_done());
  return VK_OK;
}

}  // extern "C"
