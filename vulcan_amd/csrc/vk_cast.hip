// vk_cast.hip — what arbitrary rays through a voxel-hashed volume hit first, and how far away, for gfx950 (no upstream
// counterpart: the reference casts only the pixel rays of one pinhole camera, src/tracer.cu:317-451, whose march rule this
// is, in voxel units; ref: src/volume.cu:168-191 for the chain walk. The definition is in include/vk.h at
// vk_volume_cast_rays; tests/cast_reference.py states it on the CPU and the device is held to it bit for bit).
//
// Shape: one launch on the caller's stream, one lane per ray, nothing read back. The volume is only read, every output
// element is written by its own lane, there is no atomic and no workgroup waits on another. Every loop is bounded:
// max_steps bounds the march (every turn of it counts a step) and find_block's guard bounds a chain walk. A lane keeps
// the block it is in and that block's slot (or its absence) in registers, so a step that stays in the block probes its
// nearest voxel with one pool read and no table read; near the surface, and for the hit, the cell of the point is read by
// read_cell (vk_block_walk.hpp, shared with vk_sample.hip). The lanes of a wave march rays of different lengths: the wave
// takes as many turns as its longest ray.
#include "vk_block_walk.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;

struct CastParams
{
  vk_volume v;
  int total;                    // main + excess entries = pool slots
  int count;
  int voxel_units;
  int max_steps;
  float t_min, t_max;
  const float* rays;            // [6 * count]
  const vk_transform* pose;     // device, or null
  float* t_out;                 // [count]
  int32_t* status;              // [count]
  vk_voxel* samples;            // [count], or null
  float* gradients;             // [4 * count], or null
};

__device__ __forceinline__ f3 along(f3 o, float t, f3 n) { return f3{o.x + t * n.x, o.y + t * n.y, o.z + t * n.z}; }

// vk_volume_sample's distance sample at p (the USED rule): does it exist, and its value
__device__ __forceinline__ bool distance_sample(const CastParams& P, f3 p, float& distance)
{
  const Cell c = read_cell<false, false>(P.v, P.total, p, finite3(p));
  if (c.has_d) distance = trilinear(c.distance, c.l.fx, c.l.fy, c.l.fz);
  return c.has_d;
}

// the step that leaves the absent block (bx, by, bz) through its exit face: the smallest distance to a face ahead
__device__ __forceinline__ float exit_step(f3 p, f3 n, int bx, int by, int bz)
{
  float s = INFINITY;
  if (n.x != 0.0f) s = fminf(s, ((float)(8 * bx + (n.x > 0.0f ? 8 : 0)) - p.x) / n.x);
  if (n.y != 0.0f) s = fminf(s, ((float)(8 * by + (n.y > 0.0f ? 8 : 0)) - p.y) / n.y);
  if (n.z != 0.0f) s = fminf(s, ((float)(8 * bz + (n.z > 0.0f ? 8 : 0)) - p.z) / n.z);
  return fmaxf(s, 0.0f) + 0.5f;
}

// COLOR: the colour fields of a hit are sampled (else they are 0 and no colour byte is read). GRADIENT: gradients is written.
template <bool COLOR, bool GRADIENT>
__global__ __launch_bounds__(kThreads) void cast_kernel(CastParams P)
{
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)P.count) return;
  const float voxel_length = P.v.voxel_length;
  const float tr = P.v.truncation_length / voxel_length;
  float t = P.t_min, t1 = P.t_max;
  if (!P.voxel_units)
  {
    t = t / voxel_length;
    t1 = t1 / voxel_length;
  }
  const Ray ray = load_ray(P.rays, i, P.pose, voxel_length, P.voxel_units != 0);
  const f3 o = ray.o, n = ray.n;

  int status = VK_RAY_INVALID;
  if (ray.valid)
  {
    const uint32_t* pool = reinterpret_cast<const uint32_t*>(P.v.voxels);
    bool armed = false, held = false;
    int held_x = 0, held_y = 0, held_z = 0, held_slot = -1;          // the block of the last step and its slot, -1: absent
    for (int steps = 0;; ++steps)
    {
      if (!(t < t1)) { status = VK_RAY_MISS; break; }
      if (steps == P.max_steps) { status = VK_RAY_STEPS; break; }
      const f3 p = along(o, t, n);
      if (!finite3(p)) { status = VK_RAY_MISS; break; }
      const int cx = cell_of(p.x), cy = cell_of(p.y), cz = cell_of(p.z);
      const int bx = cx >> 3, by = cy >> 3, bz = cz >> 3;
      if (!held || bx != held_x || by != held_y || bz != held_z)
      {
        int slot = -1;
        Entry main_entry;
        if (in_int16(bx, by, bz)) find_block(P.v, P.total, bx, by, bz, slot, main_entry);
        held = true;  held_x = bx;  held_y = by;  held_z = bz;  held_slot = slot;
      }
      if (held_slot < 0)
      {
        t = t + exit_step(p, n, bx, by, bz);
        continue;
      }
      const uint32_t* voxel = pool + ((size_t)held_slot * VK_BLOCK_VOXELS + (size_t)((cz & 7) * 64 + (cy & 7) * 8 + (cx & 7))) * kVoxelWords;
      const bool observed = (int16_t)(voxel[4] & 0xffffu) != 0;
      float sdf = observed ? __uint_as_float(voxel[0]) : 1.0f;      // Voxel::Empty()'s distance, as the reference reads it
      if (observed && sdf <= 0.1f && sdf >= -0.5f) distance_sample(P, p, sdf);
      if (observed && sdf > 0.0f) armed = true;
      if (observed && armed && sdf <= 0.0f)
      {
        // the refinement: the reference's two steps
        t = t + tr * sdf;
        float again;
        if (distance_sample(P, along(o, t, n), again)) t = t + tr * again;
        status = VK_RAY_HIT;
        break;
      }
      t = t + (sdf > 0.0f ? fmaxf(1.0f, tr * sdf) : 1.0f);
    }
  }

  const bool hit = status == VK_RAY_HIT;
  P.status[i] = status;
  P.t_out[i] = hit ? (P.voxel_units ? t : t * voxel_length) : 0.0f;
  if (!(P.samples || GRADIENT)) return;
  // vk_volume_sample at the hit; without one nothing exists and nothing is read
  const f3 p = along(o, t, n);
  const Cell cell = read_cell<COLOR, GRADIENT>(P.v, P.total, p, hit && finite3(p));
  if (P.samples) store_sample<COLOR>(cell, reinterpret_cast<uint32_t*>(P.samples) + i * kVoxelWords);
  if (GRADIENT) store_gradient(cell, P.gradients + i * 4);
}

template <bool COLOR, bool GRADIENT>
int launch(const CastParams& P, hipStream_t s)
{
  hipLaunchKernelGGL((cast_kernel<COLOR, GRADIENT>), dim3((unsigned)(((size_t)P.count + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // namespace

extern "C" {

int vk_volume_cast_rays(const vk_volume* v, const float* rays, int32_t count, const vk_transform* pose_dev, const vk_cast_params* p,
    float* t_out, int32_t* status, vk_voxel* samples, float* gradients, void* stream)
{
  VK_REQUIRE(v && p);
  VK_REQUIRE(volume_ok(v));
  VK_REQUIRE((p->flags & ~(VK_CAST_VOXEL_UNITS | VK_CAST_DISTANCE_ONLY)) == 0);
  VK_REQUIRE(count >= 0);
  VK_REQUIRE(rays || count == 0);
  VK_REQUIRE(t_out && status);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(gradients) & 15) == 0);
  VK_REQUIRE(p->max_steps >= 1 && p->max_steps <= 65536);
  VK_REQUIRE(__builtin_isfinite(p->t_min) && __builtin_isfinite(p->t_max) && p->t_min >= 0.0f && p->t_min < p->t_max);
  if (count == 0) return VK_OK;
  CastParams P;
  P.v = *v;
  P.total = v->main_block_count + v->excess_block_count;
  P.count = count;
  P.voxel_units = (p->flags & VK_CAST_VOXEL_UNITS) ? 1 : 0;
  P.max_steps = p->max_steps;
  P.t_min = p->t_min;
  P.t_max = p->t_max;
  P.rays = rays;
  P.pose = pose_dev;
  P.t_out = t_out;
  P.status = status;
  P.samples = samples;
  P.gradients = gradients;
  hipStream_t s = vk_s(stream);
  const bool color = samples && !(p->flags & VK_CAST_DISTANCE_ONLY);
  if (gradients) return color ? launch<true, true>(P, s) : launch<false, true>(P, s);
  return color ? launch<true, false>(P, s) : launch<false, false>(P, s);
}

}  // extern "C"
