// vk_sample.hip — the signed distance, colour and gradient of a voxel-hashed volume at arbitrary points, for gfx950
// (no upstream counterpart: the reference reads its TSDF only along camera rays, src/tracer.cu:238-299, whose trilinear
// sample this is; ref: src/volume.cu:168-191 for the chain walk. The definition is in include/vk.h at vk_volume_sample;
// tests/sample_reference.py states it on the CPU and the device is held to it bit for bit).
//
// Shape: one launch on the caller's stream, one lane per point, nothing read back. The volume is only read, every output
// element is written by its own lane, there is no atomic and no workgroup waits on another. A lane resolves its base block
// by one chain walk and walks a further chain only for a block of the cell's 2x2x2 neighbourhood that a needed lattice
// point lies in (an axis leaves the base block only where b & 7 == 7); the slots are kept in registers, so the eight
// corners cost eight pool reads and no table read of their own. The value is vk_volume_merge_posed's expression, the
// gradient vk_volume_register's (vk_block_walk.hpp).
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

typedef float vf4 __attribute__((ext_vector_type(4)));

// a lane's block lookups are eight named registers, s[k] the slot of the block at offset k (bit a: one block further
// along axis a) from the base block: an array indexed by the lane's own k would leave the register file
__device__ __forceinline__ int pick(int k, int s0, int s1, int s2, int s3, int s4, int s5, int s6, int s7)
{
  int slot = s0;
  slot = k == 1 ? s1 : slot;  slot = k == 2 ? s2 : slot;  slot = k == 3 ? s3 : slot;  slot = k == 4 ? s4 : slot;
  slot = k == 5 ? s5 : slot;  slot = k == 6 ? s6 : slot;  slot = k == 7 ? s7 : slot;
  return slot;
}

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
    const float* m = P.pose->m;
    float fwd[12];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      fwd[4 * a + 0] = m[a];
      fwd[4 * a + 1] = m[4 + a];
      fwd[4 * a + 2] = m[8 + a];
      fwd[4 * a + 3] = m[12 + a] / voxel_length;
    }
    p = apply(fwd, q0, q1, q2);
  }
  const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  const Lattice l = lattice_at(finite ? p : f3{0.0f, 0.0f, 0.0f});
  const bool far_x = l.fx != 0.0f, far_y = l.fy != 0.0f, far_z = l.fz != 0.0f;
  // the lattice points that are read: all eight for the gradient, else the USED ones
  const int wanted = GRADIENT ? 7 : (far_x ? 1 : 0) | (far_y ? 2 : 0) | (far_z ? 4 : 0);
  // the axes along which b + 1 lies in the next block
  const int leaves = ((l.bx & 7) == 7 ? 1 : 0) | ((l.by & 7) == 7 ? 2 : 0) | ((l.bz & 7) == 7 ? 4 : 0);
  const int base_x = l.bx >> 3, base_y = l.by >> 3, base_z = l.bz >> 3;

  // the blocks of the neighbourhood a wanted point lies in: offset k is one iff k is a subset of `leaves & wanted`
  int s0 = -1, s1 = -1, s2 = -1, s3 = -1, s4 = -1, s5 = -1, s6 = -1, s7 = -1;
  const int reach = leaves & wanted;
  uint32_t pending = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) pending |= (finite && (k & ~reach) == 0) ? 1u << k : 0u;
  while (pending)
  {
    const int k = __ffs(pending) - 1;
    pending &= pending - 1u;
    const int bx = base_x + (k & 1), by = base_y + ((k >> 1) & 1), bz = base_z + (k >> 2);
    int slot = -1;
    Entry main_entry;
    if (in_int16(bx, by, bz)) find_block(P.v, P.total, bx, by, bz, slot, main_entry);
    s0 = k == 0 ? slot : s0;  s1 = k == 1 ? slot : s1;  s2 = k == 2 ? slot : s2;  s3 = k == 3 ? slot : s3;
    s4 = k == 4 ? slot : s4;  s5 = k == 5 ? slot : s5;  s6 = k == 6 ? slot : s6;  s7 = k == 7 ? slot : s7;
  }

  const uint32_t* pool = reinterpret_cast<const uint32_t*>(P.v.voxels);
  float distance[8], red[8], green[8], blue[8];
  bool has_d = finite, has_c = finite, all_d = finite;
  int least_dw = 32767, least_cw = 32767;
#pragma unroll
  for (int s = 0; s < 8; ++s)
  {
    distance[s] = red[s] = green[s] = blue[s] = 0.0f;
    const bool used = (!(s & 1) || far_x) && (!(s & 2) || far_y) && (!(s & 4) || far_z);
    if (!(GRADIENT || used)) continue;
    const int nx = l.bx + (s & 1), ny = l.by + ((s >> 1) & 1), nz = l.bz + (s >> 2);
    const int slot = pick(s & leaves, s0, s1, s2, s3, s4, s5, s6, s7);
    if (slot < 0)
    {
      all_d = false;
      if (used) has_d = has_c = false;
      continue;
    }
    const uint32_t* voxel = pool + ((size_t)slot * VK_BLOCK_VOXELS + (size_t)((nz & 7) * 64 + (ny & 7) * 8 + (nx & 7))) * kVoxelWords;
    const uint32_t weights = voxel[4];
    const int dw = (int16_t)(weights & 0xffffu), cw = (int16_t)(weights >> 16);
    if (COLOR)
    {
      const vu4 head = *reinterpret_cast<const vu4*>(voxel);
      distance[s] = __uint_as_float(head.x);
      red[s] = __uint_as_float(head.y);
      green[s] = __uint_as_float(head.z);
      blue[s] = __uint_as_float(head.w);
    }
    else distance[s] = __uint_as_float(voxel[0]);
    all_d = all_d && dw != 0;
    if (used)
    {
      has_d = has_d && dw != 0;
      has_c = has_c && cw != 0;
      least_dw = vmini(least_dw, dw);
      least_cw = vmini(least_cw, cw);
    }
  }

  if (P.samples)
  {
    // a field without a sample is Voxel::Empty()'s
    uint32_t out[5] = {__float_as_uint(1.0f), 0u, 0u, 0u, 0u};
    if (has_d)
    {
      out[0] = __float_as_uint(trilinear(distance, l.fx, l.fy, l.fz));
      out[4] = (uint32_t)(uint16_t)least_dw;
    }
    if (COLOR && has_c)
    {
      out[1] = __float_as_uint(trilinear(red, l.fx, l.fy, l.fz));
      out[2] = __float_as_uint(trilinear(green, l.fx, l.fy, l.fz));
      out[3] = __float_as_uint(trilinear(blue, l.fx, l.fy, l.fz));
      out[4] |= (uint32_t)(uint16_t)least_cw << 16;
    }
    uint32_t* sample = reinterpret_cast<uint32_t*>(P.samples) + i * kVoxelWords;
    vu4 head;
    head.x = out[0];  head.y = out[1];  head.z = out[2];  head.w = out[3];
    *reinterpret_cast<vu4*>(sample) = head;
    sample[4] = out[4];
  }
  if (GRADIENT)
  {
    vf4 g = {0.0f, 0.0f, 0.0f, 0.0f};
    if (all_d)
    {
      float gx, gy, gz;
      trilinear_gradient(distance, l.fx, l.fy, l.fz, gx, gy, gz);
      g.x = gx;  g.y = gy;  g.z = gz;  g.w = 1.0f;
    }
    reinterpret_cast<vf4*>(P.gradients)[i] = g;          // one 16-byte store
  }
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
