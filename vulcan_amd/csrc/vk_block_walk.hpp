// vk_block_walk.hpp — what the operations on a voxel-hashed volume share (vk_merge.hip, vk_merge_pose.hip, vk_register.hip,
// vk_sample.hip, vk_cast.hip, vk_integrate_rays.hip, vk_carve_rays.hip; the allocation rounds are in vk_alloc_rounds.hpp beside
// it, the walk of a range ray's cells in vk_range_rays.hpp):
//   wave_add, wave_min                      sums and minima over a wave
//   voxel_rows, carry_rows, apply           the pose as three rows in voxel units, and a point through them
//   find_block, mark_chain                  the chain walk that finds a block; the one that lists a bucket's blocks
//   Ray, load_ray, finite3, cell_of, kFar   a ray in the volume's frame, and the cell of a point
//   Lattice, lattice_at, lattice_of         the lattice cell a carried point falls into
//   fill_directory, fill_directory_cells    the 4x4x4 blocks under one carried block, or side^3 from a given block, as slots in LDS
//   trilinear, trilinear_gradient           the value and gradient over a cell's eight values
//   Cell, read_cell, store_sample, store_gradient   the cell of a point read from the pool as vk_volume_sample defines it
//   volume_ok, volumes_match                the host's checks of a volume and of a pair
// The definitions are in include/vk.h at vk_volume_merge_posed (coordinates, chain walk, absent beyond the int16 range,
// the value), vk_volume_register (the gradient), vk_volume_sample (the sample of a point) and vk_volume_cast_rays (the ray).
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

// rows 0-2 of a column-major 4x4, the translation in voxels
__host__ __device__ __forceinline__ void carry_rows(const float* m, float voxel_length, float rows[12])
{
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    rows[4 * a + 0] = m[a];
    rows[4 * a + 1] = m[4 + a];
    rows[4 * a + 2] = m[8 + a];
    rows[4 * a + 3] = m[12 + a] / voxel_length;
  }
}
__device__ __forceinline__ void carry_rows(const vk_transform* t, float voxel_length, float rows[12]) { carry_rows(t->m, voxel_length, rows); }

// the host's: false when one of the twelve is not finite
inline bool voxel_rows(const float* m, float voxel_length, float* rows)
{
  for (int i = 0; i < 16; ++i)
    if ((i & 3) != 3 && !isfinite(m[i])) return false;
  carry_rows(m, voxel_length, rows);
  return true;
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

// The source blocks of one main bucket: an entry with data >= 0 that is reachable from the bucket along `next`. A link that
// leaves the table ends the chain and no chain is longer than the table (as in vk_release.hip). mark(index) per such entry;
// how many there were (0 for a thread beyond the last bucket).
template <class Mark>
__device__ __forceinline__ int mark_chain(const vk_volume& v, int total, int bucket, Mark&& mark)
{
  int blocks = 0;
  if (bucket >= v.main_block_count) return blocks;
  int index = bucket;
  for (int guard = 0; index >= 0 && index < total && guard < total; ++guard)
  {
    const Entry entry = load_entry(v.hash_entries, (uint32_t)index);
    if (entry.data >= 0 && entry.data < total)
    {
      mark(index);
      ++blocks;
    }
    index = entry.next;
  }
  return blocks;
}

constexpr int kFar = 1 << 30;                  // a coordinate is clamped here, so that the next cell is still an int

__device__ __forceinline__ bool finite3(f3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// the cell a coordinate lies in
__device__ __forceinline__ int cell_of(float p) { return vclampi(f2i(floorf(p)), -kFar, kFar); }

// Ray i of a [6 * count] array as vk_volume_cast_rays defines it: origin and unit direction in voxels, in the volume's frame.
// The origin is divided by the voxel length unless `voxel_units` and goes through the pose, the direction through its
// rotation only. `valid`: the origin within 2^30 and a finite unit direction.
struct Ray
{
  f3 o, n;
  bool valid;
};

__device__ __forceinline__ Ray load_ray(const float* rays, size_t i, const vk_transform* pose, float voxel_length, bool voxel_units)
{
  const float* x = rays + i * 6;
  float q0 = x[0], q1 = x[1], q2 = x[2];
  float d0 = x[3], d1 = x[4], d2 = x[5];
  if (!voxel_units)
  {
    q0 = q0 / voxel_length;
    q1 = q1 / voxel_length;
    q2 = q2 / voxel_length;
  }
  Ray ray;
  ray.o = f3{q0, q1, q2};
  if (pose)
  {
    float fwd[12];
    carry_rows(pose, voxel_length, fwd);
    ray.o = apply(fwd, q0, q1, q2);
    const float r0 = (fwd[0] * d0 + fwd[1] * d1) + fwd[2] * d2, r1 = (fwd[4] * d0 + fwd[5] * d1) + fwd[6] * d2,
                r2 = (fwd[8] * d0 + fwd[9] * d1) + fwd[10] * d2;
    d0 = r0;  d1 = r1;  d2 = r2;
  }
  const float len = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
  ray.n = f3{d0 / len, d1 / len, d2 / len};
  ray.valid = fabsf(ray.o.x) < (float)kFar && fabsf(ray.o.y) < (float)kFar && fabsf(ray.o.z) < (float)kFar && isfinite(len) && finite3(ray.n);
  return ray;
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
  return Lattice{vclampi(f2i(qx), -kFar, kFar), vclampi(f2i(qy), -kFar, kFar), vclampi(f2i(qz), -kFar, kFar), gx - qx, gy - qy, gz - qz};
}

// where voxel (x, y, z) of block (ox, oy, oz) samples the other volume through `rows`
__device__ __forceinline__ Lattice lattice_of(const float* rows, int ox, int oy, int oz, int x, int y, int z)
{
  return lattice_at(apply(rows, (float)(8 * ox + x) + 0.5f, (float)(8 * oy + y) + 0.5f, (float)(8 * oz + z) + 0.5f));
}

constexpr int kFootprint = 4;                  // blocks per axis under one block carried through a rigid pose
static_assert(kFootprint * kFootprint * kFootprint == kWave, "one lane per directory cell");

// One wave: the slots (-1: absent) of the side^3 blocks of `v` from block (least_x, least_y, least_z) into the wave's LDS
// `directory`, cell (rx, ry, rz) at rx + side ry + side^2 rz. The lanes stride over the cells, one chain walk per cell.
__device__ __forceinline__ void fill_directory_cells(const vk_volume& v, int total, int least_x, int least_y, int least_z, int side,
    int* directory)
{
  const int cells = side * side * side;
  for (int cell = lane_id(); cell < cells; cell += kWave)
  {
    const int sx = least_x + cell % side, sy = least_y + (cell / side) % side, sz = least_z + cell / (side * side);
    int slot = -1;
    Entry main_entry;
    if (in_int16(sx, sy, sz)) find_block(v, total, sx, sy, sz, slot, main_entry);
    directory[cell] = slot;
  }
  wave_lds_fence();
}

// One wave, eight voxels per lane (lane = 8 y + x). Under a rigid pose the lattice points of the 512 samples of block `mine`
// carried through `rows` lie in at most 4^3 blocks of `v` from the least one: lane k walks the chain of cell k once and
// leaves the slot (-1: absent) in the wave's 64-word LDS `directory`, cell (rx, ry, rz) at rx + 4 ry + 16 rz.
__device__ __forceinline__ void fill_directory(const vk_volume& v, int total, const float* rows, const Entry& mine, int* directory,
    int& least_x, int& least_y, int& least_z)
{
  const int lane = lane_id();
  least_x = least_y = least_z = INT32_MAX;
#pragma unroll
  for (int z = 0; z < 8; ++z)
  {
    const Lattice l = lattice_of(rows, mine.ox, mine.oy, mine.oz, lane & 7, lane >> 3, z);
    least_x = vmini(least_x, l.bx >> 3);
    least_y = vmini(least_y, l.by >> 3);
    least_z = vmini(least_z, l.bz >> 3);
  }
  least_x = wave_min(least_x);
  least_y = wave_min(least_y);
  least_z = wave_min(least_z);
  fill_directory_cells(v, total, least_x, least_y, least_z, kFootprint, directory);
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

// a lane's block lookups are eight named registers, s[k] the slot of the block at offset k (bit a: one block further
// along axis a) from the base block: an array indexed by the lane's own k would leave the register file
__device__ __forceinline__ int pick(int k, int s0, int s1, int s2, int s3, int s4, int s5, int s6, int s7)
{
  int slot = s0;
  slot = k == 1 ? s1 : slot;  slot = k == 2 ? s2 : slot;  slot = k == 3 ? s3 : slot;  slot = k == 4 ? s4 : slot;
  slot = k == 5 ? s5 : slot;  slot = k == 6 ? s6 : slot;  slot = k == 7 ? s7 : slot;
  return slot;
}

typedef float vf4 __attribute__((ext_vector_type(4)));

// what a point reads of the pool, vk_volume_sample's definition: the eight values of its cell (0 where a lattice point is
// not read or absent), whether the distance and the colour sample exist by the USED rule with their smallest weights, and
// whether all eight points carry a distance (the gradient's condition)
struct Cell
{
  Lattice l;
  float distance[8], red[8], green[8], blue[8];
  bool has_d, has_c, all_d;
  int least_dw, least_cw;
};

// COLOR: the colour fields are read (else they are 0 and no colour byte is read). GRADIENT: all eight lattice points are
// read, else the USED ones. A lane resolves its base block by one chain walk and walks a further chain only for a block of
// the cell's 2x2x2 neighbourhood that a wanted lattice point lies in (an axis leaves the base block only where
// b & 7 == 7); the slots are kept in registers, so the eight corners cost eight pool reads and no table read of their own.
// `finite`: p has three finite components; a point without has no sample of any kind and reads nothing.
template <bool COLOR, bool GRADIENT>
__device__ __forceinline__ Cell read_cell(const vk_volume& v, int total, f3 p, bool finite)
{
  Cell c;
  c.l = lattice_at(finite ? p : f3{0.0f, 0.0f, 0.0f});
  const Lattice& l = c.l;
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
    if (in_int16(bx, by, bz)) find_block(v, total, bx, by, bz, slot, main_entry);
    s0 = k == 0 ? slot : s0;  s1 = k == 1 ? slot : s1;  s2 = k == 2 ? slot : s2;  s3 = k == 3 ? slot : s3;
    s4 = k == 4 ? slot : s4;  s5 = k == 5 ? slot : s5;  s6 = k == 6 ? slot : s6;  s7 = k == 7 ? slot : s7;
  }

  const uint32_t* pool = reinterpret_cast<const uint32_t*>(v.voxels);
  c.has_d = c.has_c = c.all_d = finite;
  c.least_dw = c.least_cw = 32767;
#pragma unroll
  for (int s = 0; s < 8; ++s)
  {
    c.distance[s] = c.red[s] = c.green[s] = c.blue[s] = 0.0f;
    const bool used = (!(s & 1) || far_x) && (!(s & 2) || far_y) && (!(s & 4) || far_z);
    if (!(GRADIENT || used)) continue;
    const int nx = l.bx + (s & 1), ny = l.by + ((s >> 1) & 1), nz = l.bz + (s >> 2);
    const int slot = pick(s & leaves, s0, s1, s2, s3, s4, s5, s6, s7);
    if (slot < 0)
    {
      c.all_d = false;
      if (used) c.has_d = c.has_c = false;
      continue;
    }
    const uint32_t* voxel = pool + ((size_t)slot * VK_BLOCK_VOXELS + (size_t)((nz & 7) * 64 + (ny & 7) * 8 + (nx & 7))) * kVoxelWords;
    const uint32_t weights = voxel[4];
    const int dw = (int16_t)(weights & 0xffffu), cw = (int16_t)(weights >> 16);
    if (COLOR)
    {
      const vu4 head = *reinterpret_cast<const vu4*>(voxel);
      c.distance[s] = __uint_as_float(head.x);
      c.red[s] = __uint_as_float(head.y);
      c.green[s] = __uint_as_float(head.z);
      c.blue[s] = __uint_as_float(head.w);
    }
    else c.distance[s] = __uint_as_float(voxel[0]);
    c.all_d = c.all_d && dw != 0;
    if (used)
    {
      c.has_d = c.has_d && dw != 0;
      c.has_c = c.has_c && cw != 0;
      c.least_dw = vmini(c.least_dw, dw);
      c.least_cw = vmini(c.least_cw, cw);
    }
  }
  return c;
}

// the cell's sample as a vk_voxel at `sample`: a field without a sample is Voxel::Empty()'s
template <bool COLOR>
__device__ __forceinline__ void store_sample(const Cell& c, uint32_t* sample)
{
  uint32_t out[5] = {__float_as_uint(1.0f), 0u, 0u, 0u, 0u};
  if (c.has_d)
  {
    out[0] = __float_as_uint(trilinear(c.distance, c.l.fx, c.l.fy, c.l.fz));
    out[4] = (uint32_t)(uint16_t)c.least_dw;
  }
  if (COLOR && c.has_c)
  {
    out[1] = __float_as_uint(trilinear(c.red, c.l.fx, c.l.fy, c.l.fz));
    out[2] = __float_as_uint(trilinear(c.green, c.l.fx, c.l.fy, c.l.fz));
    out[3] = __float_as_uint(trilinear(c.blue, c.l.fx, c.l.fy, c.l.fz));
    out[4] |= (uint32_t)(uint16_t)c.least_cw << 16;
  }
  vu4 head;
  head.x = out[0];  head.y = out[1];  head.z = out[2];  head.w = out[3];
  *reinterpret_cast<vu4*>(sample) = head;
  sample[4] = out[4];
}

// {gx, gy, gz, 1} of a cell read with GRADIENT, or four zeros where one of the eight is missing: one 16-byte store
__device__ __forceinline__ void store_gradient(const Cell& c, float* gradient)
{
  vf4 g = {0.0f, 0.0f, 0.0f, 0.0f};
  if (c.all_d)
  {
    float gx, gy, gz;
    trilinear_gradient(c.distance, c.l.fx, c.l.fy, c.l.fz, gx, gy, gz);
    g.x = gx;  g.y = gy;  g.z = gz;  g.w = 1.0f;
  }
  *reinterpret_cast<vf4*>(gradient) = g;
}

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

// two volumes one lattice can be carried between: the same voxel and truncation length, bit for bit
inline bool volumes_match(const vk_volume* dst, const vk_volume* src)
{
  return volume_ok(dst) && volume_ok(src) && memcmp(&dst->voxel_length, &src->voxel_length, sizeof(float)) == 0 &&
         memcmp(&dst->truncation_length, &src->truncation_length, sizeof(float)) == 0;
}

}  // namespace vk
