// vk_register_rays.hip — localise a sweep of range rays in a voxel-hashed volume: Gauss-Newton on "the endpoint of a return
// lies on the surface", for gfx950 (no upstream counterpart: the reference tracks only pinhole depth images against a raycast
// keyframe; ref: src/tracker.cpp:124-163 for the loop and its end, src/color_tracker.cpp:45-95 for the step,
// src/tracer.cu:238-299 for the trilinear sample. The definition is in include/vk.h at vk_volume_register_rays;
// tests/register_rays_reference.py states it on the CPU: the per-ray terms are held to it bit for bit, the sums to the
// project's bound for a normal system, tests/test_gpu_register_rays.py).
//
// Shape: launch per stage, everything enqueued on the caller's stream, nothing read back, no exchange inside a launch and
// no wait on another workgroup anywhere. The volume is only read.
//   pass      one lane per ray, 512 per workgroup: the ray (load_range_ray), its endpoint, the endpoint's cell (read_cell:
//             the blocks of the 2x2x2 neighbourhood resolved once, their slots in registers, eight pool reads, no colour byte),
//             value and gradient (trilinear_gradient), residual and Jacobian. The workgroup's 27 + 1 sums and four counts go
//             to its own row of partials (store_partial): a row per workgroup whatever it found, so the rows and their order
//             depend on `count` alone
//   sum       one workgroup (256 lanes, 1024 beyond 1 024 rows: sum_partials gives the same bits with either): its fixed
//             order into system[48], the four counts
//   solve     one wave: register_solve_kernel (vk_register_step.hpp), vk_volume_register's
// A row stands for 512 consecutive rays and a lane holds one ray, so a sweep of 307 200 rays is 4 800 waves in 600 workgroups:
// measured, 256- and 512-wide workgroups cost the same and 1024-wide ones 8 % more on a shuffled sweep. The
// largest call (1 << 22 rays) leaves 8 192 rows for the one workgroup of the sum: sixteen rounds of sixteen loads per lane
// at 1024 lanes. Four rays per lane would quarter the rows and the waves in flight with them; the gather is latency bound.
// Every loop is bounded: a chain walk by the table size. There is no float atomic.
#include "vk_range_rays.hpp"
#include "vk_register_step.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 512;                                          // rays per workgroup = rays per row of partials
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxCount = 1 << 22;

enum { kSumSquares = 27, kMeasured = 28, kSampled = 29, kResiduals = 30, kBad = 31 };      // a partial row behind the 27 sums (four are ints)
static_assert(kBad < kSysStride, "a partial row");

struct RegisterRaysParams : RangeRays
{
  float band, inverse_voxel;
  const int32_t* state;         // device {steps, code}, or null: a pass that finds a code returns at once
  float* partials;              // workspace: [groups][kSysStride]
  // vk_volume_register_rays_terms
  float* residuals;
  float* jacobians;
  uint8_t* valid;
};

// One lane per ray. Every workgroup writes its row of partials: 27 sums, the sum of squares, four counts.
template <bool TERMS>
__global__ __launch_bounds__(kThreads) void register_rays_pass_kernel(RegisterRaysParams P)
{
  __shared__ float lds[kWaves][kSysStride];
  __shared__ int behind[kWaves][4];
  __shared__ float squared[kWaves];
  if (P.state && P.state[1]) return;              // over, for the whole grid
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  float acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.0f;
  float squares = 0.0f;
  int measured = 0, sampled = 0, residual = 0, bad = 0;
  if (i < (size_t)P.count)
  {
    const RangeRay ray = load_range_ray(P, i);
    bad = ray.kind == kInvalid ? 1 : 0;
    measured = ray.kind == kIntegrated ? 1 : 0;
    float r = 0.0f;
    float J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (measured)
    {
      const Residual t = residual_test(P.v, P.total, ray, P.band);
      sampled = t.sampled ? 1 : 0;
      if (t.residual)
      {
        residual = 1;
        r = t.D;
        const f3 e = t.e;
        const float gx = t.gx, gy = t.gy, gz = t.gz, iv = P.inverse_voxel;
        J[0] = e.y * gz - e.z * gy;  J[1] = e.z * gx - e.x * gz;  J[2] = e.x * gy - e.y * gx;
        J[3] = gx * iv;  J[4] = gy * iv;  J[5] = gz * iv;
        outer_products(J, r, acc);
        squares = r * r;
      }
    }
    if (TERMS)
    {
      P.valid[i] = (uint8_t)residual;
      P.residuals[i] = r;
#pragma unroll
      for (int k = 0; k < 6; ++k) P.jacobians[i * 6 + k] = J[k];
    }
  }
  const int wave = (int)(threadIdx.x >> 6);
  squares = wave_sum_lane63(squares);
  // the four counts are of flags: a ballot and a population count each, no lane exchange
  const int measured_here = __popcll(__ballot(measured)), sampled_here = __popcll(__ballot(sampled));
  const int residuals_here = __popcll(__ballot(residual)), bad_here = __popcll(__ballot(bad));
  if (lane_id() == 63)
  {
    squared[wave] = squares;
    behind[wave][0] = measured_here;
    behind[wave][1] = sampled_here;
    behind[wave][2] = residuals_here;
    behind[wave][3] = bad_here;
  }
  store_partial<kWaves>(acc, lds, P.partials);                // (its barrier follows the stores above)
  float* row = P.partials + (size_t)blockIdx.x * kSysStride;
  if (threadIdx.x == kSumSquares)
  {
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += squared[w];
    row[kSumSquares] = v;
  }
  if (threadIdx.x >= kMeasured && threadIdx.x <= kBad)
  {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v += behind[w][threadIdx.x - kMeasured];
    row[threadIdx.x] = __int_as_float(v);
  }
}

// The fixed-order second stage (sum_partials) into system[48], and the counts.
__global__ __launch_bounds__(1024) void register_rays_sum_kernel(const float* __restrict__ partials, int groups, const int32_t* state,
    float* __restrict__ system, int32_t* __restrict__ counts)
{
  __shared__ float slices[kSysSlices][kSysStride];
  __shared__ float sums[48];
  __shared__ int32_t totals[4];
  if (state && state[1]) return;
  if (threadIdx.x < 4) totals[threadIdx.x] = 0;
  __syncthreads();
  int mine[4] = {0, 0, 0, 0};
  for (int g = threadIdx.x; g < groups; g += blockDim.x)
  {
#pragma unroll
    for (int k = 0; k < 4; ++k) mine[k] += __float_as_int(partials[(size_t)g * kSysStride + kMeasured + k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) wave_add(&totals[k], mine[k]);
  sum_partials(partials, groups, 1, system, system + 36, slices, sums);      // (ends with a barrier)
  if (threadIdx.x == 0)
  {
    float squares = 0.0f;
    for (int k = 0; k < kSysSlices; ++k) squares += slices[k][kSumSquares];
    system[42] = squares;
    for (int i = 43; i < 48; ++i) system[i] = 0.0f;
    counts[0] = totals[0];
    counts[1] = totals[1];
    counts[2] = totals[2];
    counts[3] = totals[3];
  }
}

inline int groups_of(int count) { return (count + kThreads - 1) / kThreads; }

// the host checks and the workspace; VK_OK or VK_ERR_ARGUMENT
int prepare(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* pose_dev,
    const vk_register_rays_params* p, void* workspace, RegisterRaysParams& P)
{
  VK_REQUIRE(v && p);
  VK_REQUIRE(p->iterations >= 1 && p->iterations <= 64);
  VK_REQUIRE(p->max_abs_distance > 0.0f && p->max_abs_distance <= 1.0f);        // (false for a NaN)
  VK_REQUIRE(range_rays_arguments(v, rays, ranges, count, pose_dev, p->flags, p->r_min, p->r_max, workspace, VK_RAYS_VOXEL_UNITS,
      kMaxCount, false, false, P) == VK_OK);
  P.band = p->max_abs_distance;
  P.inverse_voxel = 1.0f / v->voxel_length;
  P.state = nullptr;
  P.partials = static_cast<float*>(workspace);
  P.residuals = P.jacobians = nullptr;
  P.valid = nullptr;
  return VK_OK;
}

int evaluate(const RegisterRaysParams& P, float* system_dev, int32_t* counts_dev, hipStream_t s)
{
  const int groups = groups_of(P.count);
  hipLaunchKernelGGL(register_rays_pass_kernel<false>, dim3(groups), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(register_rays_sum_kernel, dim3(1), dim3(groups > 1024 ? 1024 : 256), 0, s, P.partials, groups, P.state, system_dev,
      counts_dev);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // namespace

extern "C" {

size_t vk_volume_register_rays_workspace_bytes(int32_t count)
{
  if (count < 0 || count > kMaxCount) return 0;
  const int groups = groups_of(count);
  return align_up((size_t)(groups > 0 ? groups : 1) * kSysStride * sizeof(float));
}

int vk_volume_register_rays_terms(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* pose_dev,
    const vk_register_rays_params* p, float* residuals, float* jacobians, uint8_t* valid, void* workspace, void* stream)
{
  VK_REQUIRE(residuals && jacobians && valid);
  RegisterRaysParams P;
  { const int code = prepare(v, rays, ranges, count, pose_dev, p, workspace, P);  if (code != VK_OK) return code; }
  if (count == 0) return VK_OK;
  P.residuals = residuals;
  P.jacobians = jacobians;
  P.valid = valid;
  hipLaunchKernelGGL(register_rays_pass_kernel<true>, dim3(groups_of(count)), dim3(kThreads), 0, vk_s(stream), P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

int vk_volume_register_rays_system(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* pose_dev,
    const vk_register_rays_params* p, float* system_dev, int32_t* counts_dev, void* workspace, void* stream)
{
  VK_REQUIRE(system_dev && counts_dev);
  RegisterRaysParams P;
  { const int code = prepare(v, rays, ranges, count, pose_dev, p, workspace, P);  if (code != VK_OK) return code; }
  if (count == 0) return VK_OK;
  return evaluate(P, system_dev, counts_dev, vk_s(stream));
}

int vk_volume_register_rays(const vk_volume* v, const float* rays, const float* ranges, int32_t count, vk_transform* pose_dev,
    const vk_register_rays_params* p, float* system_dev, int32_t* state_dev, int32_t* counts_dev, float* update_dev, void* workspace,
    void* stream)
{
  VK_REQUIRE(system_dev && state_dev && counts_dev);
  RegisterRaysParams P;
  { const int code = prepare(v, rays, ranges, count, pose_dev, p, workspace, P);  if (code != VK_OK) return code; }
  if (count == 0) return VK_OK;
  hipStream_t s = vk_s(stream);
  P.state = state_dev;
  for (int it = 0; it < p->iterations; ++it)
  {
    { const int code = evaluate(P, system_dev, counts_dev, s);  if (code != VK_OK) return code; }
    hipLaunchKernelGGL(register_solve_kernel, dim3(1), dim3(64), 0, s, system_dev, counts_dev, pose_dev, state_dev, update_dev);
    VK_LAUNCH_CHECK();
  }
  return VK_OK;
}

}  // extern "C"
