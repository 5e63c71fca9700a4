// vk_block_walk.hpp — what the passes that carry a point into a volume's lattice share (vk_merge_pose.hip,
// vk_register.hip, vk_sample.hip): the pose as three rows in voxel units, the chain walk that finds a block, the lattice
// cell a carried point falls into, the trilinear value and gradient over a cell's eight values, and the host's checks of
// a volume. The definitions are in include/vk.h at vk_volume_merge_posed (coordinates, chain walk, absent beyond the int16
// range, the value) and vk_volume_register (the gradient).
#pragma once

#include "vk_requests.hpp"

#include <math.h>

namespace vk
{

constexpr int kVoxelWords = (int)sizeof(vk_voxel) / 4;                 // 5 dwords: distance, colour, the two weights
static_assert(sizeof(vk_voxel) == 20, "Voxel layout");

typedef uint32_t vu4 __attribute__((ext_vector_type(4), aligned(4)));   // a voxel's first 16 bytes, 4-byte aligned

// sum over the wave, then one atomic: integer sums commute
__device__ __forceinline__ void wave_add(int32_t* word, int value)
{
  for (int d = 32; d > 0; d >>= 1) value += __shfl_down(value, d);
  if (lane_id() == 0 && value) atomicAdd(word, value);
}

__device__ __forceinline__ int wave_min(int v)
{
  for (int d = 32; d > 0; d >>= 1) v = vmini(v, __shfl_xor(v, d));
  return v;
}

// row a of `r`: m[a], m[4+a], m[8+a], the translation in voxels
__device__ __forceinline__ f3 apply(const float* r, float c0, float c1, float c2)
{
  return f3{((r[0] * c0 + r[1] * c1) + r[2] * c2) + r[3], ((r[4] * c0 + r[5] * c1) + r[6] * c2) + r[7],
            ((r[8] * c0 + r[9] * c1) + r[10] * c2) + r[11]};
}

__device__ __forceinline__ bool in_int16(int x, int y, int z)
{
  return x >= -32768 && x <= 32767 && y >= -32768 && y <= 32767 && z >= -32768 && z <= 32767;
}

// the entry of block (bx, by, bz) in `v` by the chain walk of its bucket: an entry with data >= 0 and that origin (the
// empty main entry does not stand in for block (0,0,0)); -1 when absent. `main_entry`: the bucket's, for the request.
__device__ __forceinline__ int find_block(const vk_volume& v, int total, int bx, int by, int bz, int& slot, Entry& main_entry)
{
  const uint32_t bucket = block_hash(bx, by, bz, (uint32_t)v.main_block_count);
  main_entry = load_entry(v.hash_entries, bucket);
  Entry entry = main_entry;
  int at = (int)bucket;
  for (int guard = 0; guard < total; ++guard)
  {
    if (entry.data >= 0 && entry.data < total && entry_is(entry, bx, by, bz))
    {
      slot = entry.data;
      return at;
    }
    at = entry.next;
    if (at < 0 || at >= total) break;
    entry = load_entry(v.hash_entries, (uint32_t)at);
  }
  slot = -1;
  return -1;
}

struct Lattice
{
  int bx, by, bz;               // floorf(g)
  float fx, fy, fz;             // g - floorf(g)
};

// the cell of the other lattice that the carried centre p samples: g = p - 0.5f. (The clamp keeps b + 1 an int; a rigid
// pose never nears it.)
__device__ __forceinline__ Lattice lattice_at(f3 p)
{
  const float gx = p.x - 0.5f, gy = p.y - 0.5f, gz = p.z - 0.5f;
  const float qx = floorf(gx), qy = floorf(gy), qz = floorf(gz);
  constexpr int kFar = 1 << 30;
  return Lattice{vclampi(f2i(qx), -kFar, kFar), vclampi(f2i(qy), -kFar, kFar), vclampi(f2i(qz), -kFar, kFar), gx - qx, gy - qy, gz - qz};
}

// where voxel (x, y, z) of block (ox, oy, oz) samples the other volume through `rows`
__device__ __forceinline__ Lattice lattice_of(const float* rows, int ox, int oy, int oz, int x, int y, int z)
{
  return lattice_at(apply(rows, (float)(8 * ox + x) + 0.5f, (float)(8 * oy + y) + 0.5f, (float)(8 * oz + z) + 0.5f));
}

// the value, vk_volume_merge_posed's spelling: an axis with f == 0 takes its base value
__device__ __forceinline__ float lerp_axis(float f, float a, float b) { return f == 0.0f ? a : a + f * (b - a); }

// x, then y, then z over the eight values v[s], s = sx + 2 sy + 4 sz
__device__ __forceinline__ float trilinear(const float v[8], float fx, float fy, float fz)
{
  const float x00 = lerp_axis(fx, v[0], v[1]), x10 = lerp_axis(fx, v[2], v[3]), x01 = lerp_axis(fx, v[4], v[5]), x11 = lerp_axis(fx, v[6], v[7]);
  const float y0 = lerp_axis(fy, x00, x10), y1 = lerp_axis(fy, x01, x11);
  return lerp_axis(fz, y0, y1);
}

// the value and its gradient per voxel, vk_volume_register's spelling: all eight values take part on every axis
__device__ __forceinline__ float lerp(float t, float a, float b) { return a + t * (b - a); }

__device__ __forceinline__ float trilinear_gradient(const float v[8], float fx, float fy, float fz, float& gx, float& gy, float& gz)
{
  const float x00 = lerp(fx, v[0], v[1]), x10 = lerp(fx, v[2], v[3]), x01 = lerp(fx, v[4], v[5]), x11 = lerp(fx, v[6], v[7]);
  const float y0 = lerp(fy, x00, x10), y1 = lerp(fy, x01, x11);
  const float D = lerp(fz, y0, y1);
  gz = y1 - y0;
  gy = lerp(fz, x10 - x00, x11 - x01);
  gx = lerp(fz, lerp(fy, v[1] - v[0], v[3] - v[2]), lerp(fy, v[5] - v[4], v[7] - v[6]));
  return D;
}

inline size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

inline bool volume_ok(const vk_volume* v)
{
  return v && v->voxels && v->hash_entries && v->free_voxel_blocks && v->allocation_types && v->allocation_blocks &&
         v->block_visibility && v->visible_blocks && v->counters && v->main_block_count > 0 && v->excess_block_count >= 0 &&
         v->excess_block_count <= INT32_MAX - v->main_block_count && v->voxel_length > 0 && v->truncation_length > 0 &&
         // what the handle pass asks of a volume (check_volume, vk_volume.hip): refused here, before anything is enqueued
         (reinterpret_cast<uintptr_t>(v->counters) & 7) == 0 && (reinterpret_cast<uintptr_t>(v->allocation_blocks) & 7) == 0 &&
         (reinterpret_cast<uintptr_t>(v->hash_entries) & 15) == 0 && (reinterpret_cast<uintptr_t>(v->voxels) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(v->block_visibility) & 3) == 0 && (reinterpret_cast<uintptr_t>(v->allocation_types) & 15) == 0;
}

}  // namespace vk
