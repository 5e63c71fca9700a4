// vk_register.hip — register one voxel-hashed volume against another: Gauss-Newton on the TSDFs themselves, for gfx950
// (no upstream counterpart: its Volume is a process-wide singleton, src/volume.cu:17-21; ref: src/tracker.cpp:124-163 for
// the loop and its end, src/color_tracker.cpp:45-95 for the step. The definition is in include/vk.h at vk_volume_register;
// tests/register_reference.py states it on the CPU: the per-voxel terms are held to it bit for bit, the sums to the
// project's bound for a normal system, tests/test_gpu_register.py).
//
// Shape: launch per stage, everything enqueued on the caller's stream, nothing read back, no exchange inside a launch and
// no wait on another workgroup anywhere. Both volumes are only read.
//   mark      one thread per source bucket walks its chain and marks the entries that hold a block (once per call)
//   pass      one wave per source entry, four per workgroup: the block's 512 voxels, eight per lane; when one is in the
//             band, the 4x4x4 footprint in dst once into an LDS directory (the fuse pass of vk_merge_pose.hip turned
//             round: a gather from dst), then per voxel the eight neighbours, value, gradient, residual and Jacobian.
//             The workgroup's 27 + 3 sums go to its own row of partials (store_partial): a row per workgroup whatever
//             it found, so the rows and their order depend on the source's table alone
//   sum       one workgroup: sum_partials' fixed order into system[48], the integer counts
//   solve     one wave: staged_pose_step<6, -1> and rigid_from, as color_solve_kernel (register_solve_kernel,
//             vk_register_step.hpp, shared with vk_register_rays.hip)
#include "vk_block_walk.hpp"
#include "vk_register_step.hpp"

using namespace vk;

namespace
{

constexpr int kWaveThreads = 256;                                      // four waves = four source entries per workgroup
constexpr int kWavesPerGroup = kWaveThreads / kWave;

enum { cConsidered = 0, cWords = 16 };                                 // the control words
enum { kSumSquares = 27, kBanded = 28, kResiduals = 29 };              // a partial row behind the 27 sums (two are ints)
static_assert(kResiduals < kSysStride, "a partial row");

struct RegisterParams
{
  vk_volume dst, src;
  int dst_total, src_total;     // main + excess entries = pool slots
  float band, inverse_voxel;
  const vk_transform* pose;     // device
  const int32_t* state;         // device {steps, code}, or null: a pass that finds a code returns at once
  // workspace
  uint8_t* considered;          // [src_total]  1: the entry holds a source block
  int32_t* ctl;                 // [cWords]
  float* partials;              // [groups][kSysStride]
  // vk_volume_register_terms
  float* residuals;
  float* jacobians;
  uint8_t* valid;
};

// one thread per source bucket: its source blocks (mark_chain)
__global__ __launch_bounds__(256) void register_mark_kernel(RegisterParams P)
{
  const int bucket = blockIdx.x * blockDim.x + threadIdx.x;
  wave_add(&P.ctl[cConsidered], mark_chain(P.src, P.src_total, bucket, [&](int index) { P.considered[index] = 1; }));
}

// the terms of the source block at entry `index`, summed over the lane's eight voxels
template <bool TERMS>
__device__ __forceinline__ void block_terms(const RegisterParams& P, int index, int* directory, float (&acc)[27], float& squares,
    int& banded, int& residuals)
{
  const Entry mine = load_entry(P.src.hash_entries, (uint32_t)index);
  const int lane = lane_id();
  const int x = lane & 7, y = lane >> 3;
  const uint32_t* block = reinterpret_cast<const uint32_t*>(P.src.voxels) + (size_t)mine.data * VK_BLOCK_VOXELS * kVoxelWords;
  const float band = P.band;
  uint32_t in_band = 0u;
#pragma unroll
  for (int z = 0; z < 8; ++z)
  {
    const uint32_t* voxel = block + (size_t)(z * 64 + lane) * kVoxelWords;
    const float distance = __uint_as_float(voxel[0]);
    const bool in = (int16_t)(voxel[4] & 0xffffu) != 0 && fabsf(distance) < band;
    in_band |= (in ? 1u : 0u) << z;
    banded += __popcll(__ballot(in ? 1 : 0));
  }
  if (banded == 0) return;                        // (the same for the whole wave) dst is not touched

  float fwd[12];
  carry_rows(P.pose, P.dst.voxel_length, fwd);
  int least_x, least_y, least_z;
  fill_directory(P.dst, P.dst_total, fwd, mine, directory, least_x, least_y, least_z);

  const uint32_t* dst_pool = reinterpret_cast<const uint32_t*>(P.dst.voxels);
#pragma unroll 1
  for (int z = 0; z < 8; ++z)
  {
    if (!((in_band >> z) & 1u)) continue;
    const f3 p = apply(fwd, (float)(8 * mine.ox + x) + 0.5f, (float)(8 * mine.oy + y) + 0.5f, (float)(8 * mine.oz + z) + 0.5f);
    const Lattice l = lattice_at(p);
    float v[8];
    bool present = true;
#pragma unroll
    for (int k = 0; k < 8; ++k)
    {
      v[k] = 0.0f;
      const int nx = l.bx + (k & 1), ny = l.by + ((k >> 1) & 1), nz = l.bz + (k >> 2);
      const int rx = (nx >> 3) - least_x, ry = (ny >> 3) - least_y, rz = (nz >> 3) - least_z;
      int slot = -1;
      if (rx >= 0 && rx < kFootprint && ry >= 0 && ry < kFootprint && rz >= 0 && rz < kFootprint)
        slot = directory[rx + kFootprint * ry + kFootprint * kFootprint * rz];
      if (slot < 0)
      {
        present = false;
        continue;
      }
      const uint32_t* voxel = dst_pool + ((size_t)slot * VK_BLOCK_VOXELS + (size_t)((nz & 7) * 64 + (ny & 7) * 8 + (nx & 7))) * kVoxelWords;
      v[k] = __uint_as_float(voxel[0]);
      present = present && (int16_t)(voxel[4] & 0xffffu) != 0;
    }
    if (!present) continue;
    float gx, gy, gz;
    const float D = trilinear_gradient(v, l.fx, l.fy, l.fz, gx, gy, gz);
    if (!(fabsf(D) < band)) continue;
    const size_t at = (size_t)(z * 64 + lane);
    const float r = D - __uint_as_float(block[at * kVoxelWords]);
    const float iv = P.inverse_voxel;
    const float J[6] = {p.y * gz - p.z * gy, p.z * gx - p.x * gz, p.x * gy - p.y * gx, gx * iv, gy * iv, gz * iv};
    if (TERMS)
    {
      const size_t out = (size_t)mine.data * VK_BLOCK_VOXELS + at;
      P.valid[out] = 1;
      P.residuals[out] = r;
#pragma unroll
      for (int i = 0; i < 6; ++i) P.jacobians[out * 6 + i] = J[i];
    }
    float term[27];
    outer_products(J, r, term);
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] += term[i];
    squares += r * r;
    ++residuals;
  }
}

// One wave per source entry. Every workgroup writes its row of partials: 27 sums, the sum of squares, two counts.
template <bool TERMS>
__global__ __launch_bounds__(kWaveThreads) void register_pass_kernel(RegisterParams P)
{
  __shared__ int directory[kWavesPerGroup][kWave];
  __shared__ float lds[kWavesPerGroup][kSysStride];
  __shared__ float behind[kWavesPerGroup][4];
  if (P.state && P.state[1]) return;              // over, for the whole grid
  const int wave = (int)(threadIdx.x >> 6);
  const int index = blockIdx.x * kWavesPerGroup + wave;
  float acc[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = 0.0f;
  float squares = 0.0f;
  int banded = 0, residuals = 0;
  if (index < P.src_total && P.considered[index] == 1) block_terms<TERMS>(P, index, directory[wave], acc, squares, banded, residuals);
  squares = wave_sum_lane63(squares);
  for (int d = 32; d > 0; d >>= 1) residuals += __shfl_xor(residuals, d);
  if (lane_id() == 63)
  {
    behind[wave][0] = squares;
    behind[wave][1] = __int_as_float(banded);     // (a wave-wide count already)
    behind[wave][2] = __int_as_float(residuals);
  }
  store_partial<kWavesPerGroup>(acc, lds, P.partials);        // (its barrier follows the stores above)
  float* row = P.partials + (size_t)blockIdx.x * kSysStride;
  if (threadIdx.x == kSumSquares)
  {
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < kWavesPerGroup; ++w) v += behind[w][0];
    row[kSumSquares] = v;
  }
  if (threadIdx.x == kBanded || threadIdx.x == kResiduals)
  {
    int v = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerGroup; ++w) v += __float_as_int(behind[w][threadIdx.x - kBanded + 1]);
    row[threadIdx.x] = __int_as_float(v);
  }
}

// The fixed-order second stage (sum_partials) into system[48], and the counts.
__global__ __launch_bounds__(256) void register_sum_kernel(const float* __restrict__ partials, int groups, const int32_t* __restrict__ ctl,
    const int32_t* state, float* __restrict__ system, int32_t* __restrict__ counts)
{
  __shared__ float slices[kSysSlices][kSysStride];
  __shared__ float sums[48];
  __shared__ int32_t totals[2];
  if (state && state[1]) return;
  if (threadIdx.x < 2) totals[threadIdx.x] = 0;
  __syncthreads();
  int banded = 0, residuals = 0;
  for (int g = threadIdx.x; g < groups; g += blockDim.x)
  {
    banded += __float_as_int(partials[(size_t)g * kSysStride + kBanded]);
    residuals += __float_as_int(partials[(size_t)g * kSysStride + kResiduals]);
  }
  wave_add(&totals[0], banded);
  wave_add(&totals[1], residuals);
  sum_partials(partials, groups, 1, system, system + 36, slices, sums);      // (ends with a barrier)
  if (threadIdx.x == 0)
  {
    float squares = 0.0f;
    for (int k = 0; k < kSysSlices; ++k) squares += slices[k][kSumSquares];
    system[42] = squares;
    for (int i = 43; i < 48; ++i) system[i] = 0.0f;
    counts[0] = ctl[cConsidered];
    counts[1] = totals[0];
    counts[2] = totals[1];
    counts[3] = 0;
  }
}

inline int groups_of(int src_total) { return (src_total + kWavesPerGroup - 1) / kWavesPerGroup; }

// the host checks and the workspace; VK_OK or VK_ERR_ARGUMENT
int prepare(const vk_volume* dst, const vk_volume* src, const vk_transform* pose_dev, const vk_register_params* p, void* workspace,
    RegisterParams& P)
{
  VK_REQUIRE(dst && src && pose_dev && p && workspace);
  VK_REQUIRE(volumes_match(dst, src));
  VK_REQUIRE(p->flags == 0);
  VK_REQUIRE(p->iterations >= 1 && p->iterations <= 64);
  VK_REQUIRE(p->max_abs_distance > 0.0f && p->max_abs_distance <= 1.0f);        // (false for a NaN)
  P.dst = *dst;
  P.src = *src;
  P.dst_total = dst->main_block_count + dst->excess_block_count;
  P.src_total = src->main_block_count + src->excess_block_count;
  P.band = p->max_abs_distance;
  P.inverse_voxel = 1.0f / dst->voxel_length;
  P.pose = pose_dev;
  P.state = nullptr;
  char* at = static_cast<char*>(workspace);
  P.considered = reinterpret_cast<uint8_t*>(at);    at += align_up((size_t)P.src_total);
  P.ctl = reinterpret_cast<int32_t*>(at);           at += align_up(cWords * sizeof(int32_t));
  P.partials = reinterpret_cast<float*>(at);
  P.residuals = P.jacobians = nullptr;
  P.valid = nullptr;
  return VK_OK;
}

// the list of source blocks: once per call
int mark_source(const RegisterParams& P, hipStream_t s)
{
  VK_CHECK(hipMemsetAsync(P.considered, 0, align_up((size_t)P.src_total) + align_up(cWords * sizeof(int32_t)), s));
  hipLaunchKernelGGL(register_mark_kernel, dim3((P.src.main_block_count + 255) / 256), dim3(256), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

int evaluate(const RegisterParams& P, float* system_dev, int32_t* counts_dev, hipStream_t s)
{
  const int groups = groups_of(P.src_total);
  hipLaunchKernelGGL(register_pass_kernel<false>, dim3(groups), dim3(kWaveThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  hipLaunchKernelGGL(register_sum_kernel, dim3(1), dim3(256), 0, s, P.partials, groups, P.ctl, P.state, system_dev, counts_dev);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // namespace

extern "C" {

size_t vk_volume_register_workspace_bytes(int32_t src_main, int32_t src_excess)
{
  if (src_main <= 0 || src_excess < 0) return 0;
  const size_t src_total = (size_t)src_main + (size_t)src_excess;
  if (src_total > (size_t)INT32_MAX) return 0;
  return align_up(src_total) + align_up(cWords * sizeof(int32_t)) + align_up((size_t)groups_of((int)src_total) * kSysStride * sizeof(float));
}

int vk_volume_register_terms(const vk_volume* dst, const vk_volume* src, const vk_transform* pose_dev, const vk_register_params* p,
    float* residuals, float* jacobians, uint8_t* valid, void* workspace, void* stream)
{
  VK_REQUIRE(residuals && jacobians && valid);
  RegisterParams P;
  { const int code = prepare(dst, src, pose_dev, p, workspace, P);  if (code != VK_OK) return code; }
  hipStream_t s = vk_s(stream);
  const size_t voxels = (size_t)P.src_total * VK_BLOCK_VOXELS;
  P.residuals = residuals;
  P.jacobians = jacobians;
  P.valid = valid;
  VK_CHECK(hipMemsetAsync(residuals, 0, voxels * sizeof(float), s));
  VK_CHECK(hipMemsetAsync(jacobians, 0, voxels * 6 * sizeof(float), s));
  VK_CHECK(hipMemsetAsync(valid, 0, voxels, s));
  { const int code = mark_source(P, s);  if (code != VK_OK) return code; }
  hipLaunchKernelGGL(register_pass_kernel<true>, dim3(groups_of(P.src_total)), dim3(kWaveThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

int vk_volume_register_system(const vk_volume* dst, const vk_volume* src, const vk_transform* pose_dev, const vk_register_params* p,
    float* system_dev, int32_t* counts_dev, void* workspace, void* stream)
{
  VK_REQUIRE(system_dev && counts_dev);
  RegisterParams P;
  { const int code = prepare(dst, src, pose_dev, p, workspace, P);  if (code != VK_OK) return code; }
  hipStream_t s = vk_s(stream);
  { const int code = mark_source(P, s);  if (code != VK_OK) return code; }
  return evaluate(P, system_dev, counts_dev, s);
}

int vk_volume_register(const vk_volume* dst, const vk_volume* src, vk_transform* pose_dev, const vk_register_params* p,
    float* system_dev, int32_t* state_dev, int32_t* counts_dev, float* update_dev, void* workspace, void* stream)
{
  VK_REQUIRE(system_dev && state_dev && counts_dev);
  RegisterParams P;
  { const int code = prepare(dst, src, pose_dev, p, workspace, P);  if (code != VK_OK) return code; }
  hipStream_t s = vk_s(stream);
  P.state = state_dev;
  { const int code = mark_source(P, s);  if (code != VK_OK) return code; }
  for (int it = 0; it < p->iterations; ++it)
  {
    { const int code = evaluate(P, system_dev, counts_dev, s);  if (code != VK_OK) return code; }
    hipLaunchKernelGGL(register_solve_kernel, dim3(1), dim3(64), 0, s, system_dev, counts_dev, pose_dev, state_dev, update_dev);
    VK_LAUNCH_CHECK();
  }
  return VK_OK;
}

}  // extern "C"
