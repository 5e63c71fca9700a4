// vk_range_rays.hpp — what the operations along range rays share (vk_integrate_rays.hip, vk_carve_rays.hip):
//   RangeRay, load_range_ray     vk_volume_cast_rays' ray with its range in voxels, and what kind of ray it is
//   axis_setup, walk             the exact traversal of the cells a ray crosses between two distances along it
//   Held                         the block of the last visited cell and its slot, so that a chain is walked once per block
// The definitions are in include/vk.h at vk_volume_integrate_rays (the ray, the walk); vk_volume_carve_rays walks the same
// cells between other ends. Every float expression keeps the order and grouping vk.h gives it.
#pragma once

#include "vk_block_walk.hpp"

namespace vk
{

constexpr int kMaxGuardCells = 1024;         // ceilf(tb - ta) saturates here; tb - ta <= 4 tr <= 256, so it never does

enum { kIntegrated = 0, kNoMeasurement = 1, kInvalid = 2 };

// vk_volume_cast_rays' ray (load_ray), and its range
struct RangeRay : Ray
{
  float r;                      // the range in voxels
  int kind;
};

// ray i of `rays` with range i of `ranges`: a valid ray has a measurement iff r_min <= range <= r_max
__device__ __forceinline__ RangeRay load_range_ray(const float* rays, const float* ranges, size_t i, const vk_transform* pose,
    float voxel_length, bool voxel_units, float r_min, float r_max)
{
  RangeRay ray;
  static_cast<Ray&>(ray) = load_ray(rays, i, pose, voxel_length, voxel_units);
  const float range = ranges[i];
  ray.r = voxel_units ? range : range / voxel_length;
  const bool measured = r_min <= range && range <= r_max;             // false for a NaN
  ray.kind = ray.valid ? (measured ? kIntegrated : kNoMeasurement) : kInvalid;
  return ray;
}

// the first crossing along one axis and the distance between crossings: +infinity for an axis the ray does not move along
__device__ __forceinline__ void axis_setup(float ta, float p, float n, int c, int& step, float& tmax, float& tdelta)
{
  step = n > 0.0f ? 1 : (n < 0.0f ? -1 : 0);
  tmax = tdelta = INFINITY;
  if (n > 0.0f)
  {
    tmax = ta + ((float)(c + 1) - p) / n;
    tdelta = 1.0f / n;
  }
  else if (n < 0.0f)
  {
    tmax = ta + ((float)c - p) / n;
    tdelta = 1.0f / fabsf(n);
  }
}

// The exact traversal of the cells the ray crosses between ta and tb: visit(cx, cy, cz, least) per cell, at most G of them;
// `least` is the distance at which the walk leaves the cell, the smallest tmax right after the visit.
template <class Visit>
__device__ __forceinline__ void walk(const Ray& ray, float ta, float tb, Visit&& visit)
{
  const float px = ray.o.x + ta * ray.n.x, py = ray.o.y + ta * ray.n.y, pz = ray.o.z + ta * ray.n.z;
  int cx = cell_of(px), cy = cell_of(py), cz = cell_of(pz);
  int sx, sy, sz;
  float mx, my, mz, dx, dy, dz;
  axis_setup(ta, px, ray.n.x, cx, sx, mx, dx);
  axis_setup(ta, py, ray.n.y, cy, sy, my, dy);
  axis_setup(ta, pz, ray.n.z, cz, sz, mz, dz);
  const int guard = 3 * (vclampi(f2i(ceilf(tb - ta)), 0, kMaxGuardCells) + 2);
  for (int turn = 0; turn < guard; ++turn)
  {
    // the axis of the smallest tmax, x before y before z on a tie (a NaN is never the smaller)
    int axis = 0;
    float least = mx;
    if (my < least) { axis = 1;  least = my; }
    if (mz < least) { axis = 2;  least = mz; }
    visit(cx, cy, cz, least);
    if (!(least <= tb)) break;
    if (axis == 0) { cx += sx;  mx = mx + dx; }
    else if (axis == 1) { cy += sy;  my = my + dy; }
    else { cz += sz;  mz = mz + dz; }
  }
}

// the block of the last visited cell and its slot (-1: absent, or beyond the int16 range), kept across the cells of a walk
struct Held
{
  bool any = false, inside = false;
  int x = 0, y = 0, z = 0, slot = -1;
  Entry main_entry;

  // true when (bx, by, bz) is another block than the last: the chain was walked
  __device__ __forceinline__ bool move_to(const vk_volume& v, int total, int bx, int by, int bz)
  {
    if (any && bx == x && by == y && bz == z) return false;
    any = true;  x = bx;  y = by;  z = bz;
    inside = in_int16(bx, by, bz);
    slot = -1;
    if (inside) find_block(v, total, bx, by, bz, slot, main_entry);
    return true;
  }
};

}  // namespace vk
