// vk_score_poses.hip — score many candidate sensor poses for one sweep of range rays: vk_volume_register_rays' residual test
// at every (pose, ray) pair, and the pose that explains the sweep best, for gfx950 (no upstream counterpart: the reference
// tracks only pinhole depth images against a raycast keyframe; ref: src/tracker.cpp:124-163 for the loop whose start this
// finds, src/color_tracker.cpp:45-95 for the step, src/tracer.cu:238-299 for the trilinear sample. The definition is in
// include/vk.h at vk_volume_score_poses; tests/score_poses_reference.py states it on the CPU and the device is held to it
// bit for bit, sums included: they are integers, tests/test_gpu_score_poses.py).
//
// The work is a product, poses x rays. Shape: A LANE PER RAY, LOOPING OVER A TILE OF POSES (DESIGN.md §20 argues it against a
// lane per pose). A workgroup owns 256 consecutive rays x 8 consecutive poses:
//   pass      the pose of a turn of the loop is the same for the whole wave, so its twelve numbers are scalar loads into
//             SGPRs; the lane's ray is loop-invariant (seven floats, its division by the voxel length included), and
//             neighbouring lanes' endpoints are neighbouring pixels' endpoints, so the gather of a turn touches neighbouring
//             voxels. Per pose a wave pays four ballots and two 32-bit DPP sums (a term <= 2^20, 64 lanes: <= 2^26); lane 63
//             leaves the six numbers in LDS; behind the loop eight lanes add the four waves and each writes one partial
//             vk_pose_score, whatever was found, to the workspace at [ray tile][pose]
//   sum       32 poses x 8 slices of the ray tiles per workgroup: 1 KiB of consecutive partials per slice and turn, int64
//             sums, the slices added through LDS; every vk_pose_score up to pose_count is written, nothing beyond
//   best      one workgroup of 1 024 lanes: the total order (residuals down, sum_abs up, index up) per lane, wave, workgroup;
//             32 lanes copy the pose's 128 bytes
// Everything is enqueued on the caller's stream, nothing is read back, no workgroup waits on another, there is no atomic at
// all, and a chain walk is bounded by the table size. The volume, the rays, the ranges and the poses are only read.
#include "vk_range_rays.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;                  // rays per workgroup
constexpr int kWaves = kThreads / kWave;
constexpr int kPoseTile = 8;                   // poses per workgroup
constexpr int kMaxCount = 1 << 22;             // vk_volume_register_rays'
constexpr int kMaxPoses = 1 << 16;
constexpr int64_t kMaxPairs = (int64_t)1 << 28;
constexpr int kSumPoses = 32, kSumSlices = 8;  // the sum kernel's workgroup: 256 lanes
constexpr int kBestThreads = 1024;
constexpr float kUnit = 1048576.0f;            // 2^20: the sums' unit

static_assert(sizeof(vk_pose_score) == 32 && sizeof(vk_score_poses_params) == 24, "ABI");
static_assert(kPoseTile <= kWave && kSumPoses * kSumSlices == kThreads, "shapes");

struct ScorePosesParams : RangeRays   // (pose: the first of the candidates, device [pose_count])
{
  int pose_count;
  float band;
  vk_pose_score* partials;      // workspace: [ray tiles][pose_count]
};

// One lane per ray, a loop over the workgroup's poses: blockIdx.x the ray tile, blockIdx.y the pose tile.
__global__ __launch_bounds__(kThreads) void score_poses_pass_kernel(ScorePosesParams P)
{
  __shared__ int32_t found[kWaves][kPoseTile][6];
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < (size_t)P.count;
  const size_t at = live ? i : (size_t)P.count - 1;          // a lane past the sweep reads the last ray and counts nothing
  const int first = (int)blockIdx.y * kPoseTile;
  const int poses_here = vmini(kPoseTile, P.pose_count - first);
  const int wave = (int)(threadIdx.x >> 6);
  for (int k = 0; k < poses_here; ++k)
  {
    const RangeRay ray = load_range_ray(P, at, P.pose + (first + k));
    const bool bad = live && ray.kind == kInvalid;
    const bool measured = live && ray.kind == kIntegrated;
    bool sampled = false, residual = false;
    int term_abs = 0, term_square = 0;
    if (measured)
    {
      const Residual t = residual_test(P.v, P.total, ray, P.band);       // (its gradient is dead code here)
      sampled = t.sampled;
      residual = t.residual;
      if (residual)
      {
        term_abs = (int)rintf(fabsf(t.D) * kUnit);           // < 2^20: band <= 1
        term_square = (int)rintf((t.D * t.D) * kUnit);
      }
    }
    // the four counts are of flags: a ballot and a population count each; the two sums fit 32 bits inside a wave
    const int measured_here = __popcll(__ballot(measured)), sampled_here = __popcll(__ballot(sampled));
    const int residuals_here = __popcll(__ballot(residual)), bad_here = __popcll(__ballot(bad));
    term_abs = wave_sum_lane63(term_abs);
    term_square = wave_sum_lane63(term_square);
    if (lane_id() == 63)
    {
      int32_t* row = found[wave][k];
      row[0] = measured_here;  row[1] = sampled_here;  row[2] = residuals_here;  row[3] = bad_here;
      row[4] = term_abs;  row[5] = term_square;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < poses_here)
  {
    const int k = (int)threadIdx.x;
    vk_pose_score out = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
    {
      out.measured += found[w][k][0];  out.sampled += found[w][k][1];  out.residuals += found[w][k][2];  out.invalid += found[w][k][3];
      out.sum_abs += found[w][k][4];  out.sum_squares += found[w][k][5];
    }
    P.partials[(size_t)blockIdx.x * P.pose_count + (size_t)(first + k)] = out;
  }
}

// scores[pose] = the sum over the ray tiles of partials[tile][pose]: integers, so the order is free
__global__ __launch_bounds__(kThreads) void score_poses_sum_kernel(const vk_pose_score* __restrict__ partials, int tiles, int pose_count,
    vk_pose_score* __restrict__ scores)
{
  __shared__ vk_pose_score slices[kSumSlices][kSumPoses];
  const int column = (int)threadIdx.x & (kSumPoses - 1), slice = (int)threadIdx.x / kSumPoses;
  const int pose = (int)blockIdx.x * kSumPoses + column;
  vk_pose_score mine = {0, 0, 0, 0, 0, 0};
  if (pose < pose_count)
    for (int t = slice; t < tiles; t += kSumSlices)
    {
      const vk_pose_score part = partials[(size_t)t * pose_count + pose];
      mine.measured += part.measured;  mine.sampled += part.sampled;  mine.residuals += part.residuals;  mine.invalid += part.invalid;
      mine.sum_abs += part.sum_abs;  mine.sum_squares += part.sum_squares;
    }
  slices[slice][column] = mine;
  __syncthreads();
  if (slice == 0 && pose < pose_count)
  {
    vk_pose_score out = slices[0][column];
#pragma unroll
    for (int s = 1; s < kSumSlices; ++s)
    {
      const vk_pose_score& part = slices[s][column];
      out.measured += part.measured;  out.sampled += part.sampled;  out.residuals += part.residuals;  out.invalid += part.invalid;
      out.sum_abs += part.sum_abs;  out.sum_squares += part.sum_squares;
    }
    scores[pose] = out;
  }
}

// the total order of vk_volume_score_poses_best: more residuals, then a smaller sum_abs, then a smaller index
struct Candidate
{
  int residuals;                // -1: none
  int64_t sum_abs;
  int index;
};

__device__ __forceinline__ bool ahead(const Candidate& a, const Candidate& b)
{
  if (a.residuals != b.residuals) return a.residuals > b.residuals;
  if (a.sum_abs != b.sum_abs) return a.sum_abs < b.sum_abs;
  return a.index < b.index;
}

__global__ __launch_bounds__(kBestThreads) void score_poses_best_kernel(const vk_pose_score* __restrict__ scores,
    const vk_transform* poses, int pose_count, int min_residuals, int32_t* __restrict__ best, vk_transform* pose_out)
{
  __shared__ Candidate leaders[kBestThreads / kWave];
  __shared__ int chosen;
  Candidate mine = {-1, 0, INT32_MAX};
  for (int k = (int)threadIdx.x; k < pose_count; k += kBestThreads)
  {
    const Candidate here = {scores[k].residuals, scores[k].sum_abs, k};
    if (ahead(here, mine)) mine = here;
  }
  for (int d = 32; d > 0; d >>= 1)
  {
    const Candidate other = {__shfl_xor(mine.residuals, d), (int64_t)__shfl_xor((long long)mine.sum_abs, d), __shfl_xor(mine.index, d)};
    if (ahead(other, mine)) mine = other;
  }
  if (lane_id() == 0) leaders[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    Candidate first = leaders[0];
    for (int w = 1; w < kBestThreads / kWave; ++w)
      if (ahead(leaders[w], first)) first = leaders[w];
    chosen = first.residuals >= min_residuals ? first.index : -1;      // (pose_count >= 1: a first always exists)
    best[0] = chosen;
  }
  __syncthreads();
  const int k = chosen;
  if (k >= 0 && threadIdx.x < sizeof(vk_transform) / sizeof(float))
    reinterpret_cast<float*>(pose_out)[threadIdx.x] = reinterpret_cast<const float*>(poses + k)[threadIdx.x];
}

inline int tiles_of(int count) { return (count + kThreads - 1) / kThreads; }

inline bool shape_ok(int32_t count, int32_t pose_count)
{
  return count >= 0 && count <= kMaxCount && pose_count >= 1 && pose_count <= kMaxPoses && (int64_t)count * pose_count <= kMaxPairs;
}

}  // namespace

extern "C" {

size_t vk_volume_score_poses_workspace_bytes(int32_t count, int32_t pose_count)
{
  if (!shape_ok(count, pose_count)) return 0;
  const int tiles = tiles_of(count);
  return align_up((size_t)(tiles > 0 ? tiles : 1) * (size_t)pose_count * sizeof(vk_pose_score));
}

int vk_volume_score_poses(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* poses_dev,
    int32_t pose_count, const vk_score_poses_params* p, vk_pose_score* scores_dev, void* workspace, void* stream)
{
  VK_REQUIRE(v && p && scores_dev);
  VK_REQUIRE(p->min_residuals >= 1);
  VK_REQUIRE(p->max_abs_distance > 0.0f && p->max_abs_distance <= 1.0f);        // (false for a NaN)
  VK_REQUIRE(shape_ok(count, pose_count));
  ScorePosesParams P;
  VK_REQUIRE(range_rays_arguments(v, rays, ranges, count, poses_dev, p->flags, p->r_min, p->r_max, workspace, VK_RAYS_VOXEL_UNITS,
      kMaxCount, false, false, P) == VK_OK);
  if (count == 0) return VK_OK;
  P.pose_count = pose_count;
  P.band = p->max_abs_distance;
  P.partials = static_cast<vk_pose_score*>(workspace);
  hipStream_t s = vk_s(stream);
  const int tiles = tiles_of(count);
  hipLaunchKernelGGL(score_poses_pass_kernel, dim3(tiles, (pose_count + kPoseTile - 1) / kPoseTile), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_poses_sum_kernel, dim3((pose_count + kSumPoses - 1) / kSumPoses), dim3(kThreads), 0, s, P.partials, tiles,
      pose_count, scores_dev);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

int vk_volume_score_poses_best(const vk_pose_score* scores_dev, const vk_transform* poses_dev, int32_t pose_count,
    const vk_score_poses_params* p, int32_t* best_dev, vk_transform* pose_out_dev, void* stream)
{
  VK_REQUIRE(scores_dev && poses_dev && p && best_dev && pose_out_dev);
  VK_REQUIRE((p->flags & ~VK_RAYS_VOXEL_UNITS) == 0);
  VK_REQUIRE(p->min_residuals >= 1);
  VK_REQUIRE(pose_count >= 1 && pose_count <= kMaxPoses);
  hipLaunchKernelGGL(score_poses_best_kernel, dim3(1), dim3(kBestThreads), 0, vk_s(stream), scores_dev, poses_dev, pose_count,
      p->min_residuals, best_dev, pose_out_dev);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // extern "C"
