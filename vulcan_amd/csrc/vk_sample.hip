// vk_sample.hip — the signed distance, colour and gradient of a voxel-hashed volume at arbitrary points, for gfx950
// (no upstream counterpart: the reference reads its TSDF only along camera rays, src/tracer.cu:238-299, whose trilinear
// sample this is; ref: src/volume.cu:168-191 for the chain walk. The definition is in include/vk.h at vk_volume_sample;
// tests/sample_reference.py states it on the CPU and the device is held to it bit for bit).
//
// Shape: one launch on the caller's stream, one lane per point, nothing read back. The volume is only read, every output
// element is written by its own lane, there is no atomic and no workgroup waits on another. The cell of a point is read
// by read_cell (vk_block_walk.hpp, shared with vk_cast.hip): the needed blocks of the 2x2x2 neighbourhood resolved once,
// their slots in registers. The value is vk_volume_merge_posed's expression, the gradient vk_volume_register's.
#include "vk_block_walk.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;

struct SampleParams
{
  vk_volume v;
  int total;                    // main + excess entries = pool slots
  int count;
  int voxel_units;
  const float* points;          // [3 * count]
  const vk_transform* pose;     // device, or null
  vk_voxel* samples;            // [count], or null
  float* gradients;             // [4 * count], or null
};

// COLOR: the colour fields are sampled (else they are 0 and no colour byte is read). GRADIENT: gradients is written.
template <bool COLOR, bool GRADIENT>
__global__ __launch_bounds__(kThreads) void sample_kernel(SampleParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)P.count) return;
  const float* x = P.points + i * 3;
  float q0 = x[0], q1 = x[1], q2 = x[2];
  const float voxel_length = P.v.voxel_length;
  if (!P.voxel_units)
  {
    q0 = q0 / voxel_length;
    q1 = q1 / voxel_length;
    q2 = q2 / voxel_length;
  }
  f3 p = f3{q0, q1, q2};
  if (P.pose)
  {
    float fwd[12];
    carry_rows(P.pose, voxel_length, fwd);
    p = apply(fwd, q0, q1, q2);
  }
  const Cell cell = read_cell<COLOR, GRADIENT>(P.v, P.total, p, finite3(p));
  if (P.samples) store_sample<COLOR>(cell, reinterpret_cast<uint32_t*>(P.samples) + i * kVoxelWords);
  if (GRADIENT) store_gradient(cell, P.gradients + i * 4);
}

template <bool COLOR, bool GRADIENT>
int launch(const SampleParams& P, hipStream_t s)
{
  hipLaunchKernelGGL((sample_kernel<COLOR, GRADIENT>), dim3((unsigned)(((size_t)P.count + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // namespace

extern "C" {

int vk_volume_sample(const vk_volume* v, const float* points, int32_t count, const vk_transform* pose_dev, const vk_sample_params* p,
    vk_voxel* samples, float* gradients, void* stream)
{
  VK_REQUIRE(v && p);
  VK_REQUIRE(volume_ok(v));
  VK_REQUIRE((p->flags & ~(VK_SAMPLE_VOXEL_UNITS | VK_SAMPLE_DISTANCE_ONLY)) == 0);
  VK_REQUIRE(count >= 0);
  VK_REQUIRE(points || count == 0);
  VK_REQUIRE(samples || gradients);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(gradients) & 15) == 0);
  if (count == 0) return VK_OK;
  SampleParams P;
  P.v = *v;
  P.total = v->main_block_count + v->excess_block_count;
  P.count = count;
  P.voxel_units = (p->flags & VK_SAMPLE_VOXEL_UNITS) ? 1 : 0;
  P.points = points;
  P.pose = pose_dev;
  P.samples = samples;
  P.gradients = gradients;
  hipStream_t s = vk_s(stream);
  const bool color = samples && !(p->flags & VK_SAMPLE_DISTANCE_ONLY);
  if (gradients) return color ? launch<true, true>(P, s) : launch<false, true>(P, s);
  return color ? launch<true, false>(P, s) : launch<false, false>(P, s);
}

}  // extern "C"
