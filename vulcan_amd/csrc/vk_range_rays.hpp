// vk_range_rays.hpp — what the operations along range rays share (vk_integrate_rays.hip, vk_carve_rays.hip, vk_color_rays.hip,
// vk_register_rays.hip, vk_score_poses.hip):
//   RangeRays, range_rays_arguments   what every such call carries into its kernels, and the host's checks that fill it
//   RangeRay, load_range_ray          vk_volume_cast_rays' ray with its range in voxels, and what kind of ray it is
//   axis_setup, least_axis, walk      the exact traversal of the cells a ray crosses between two distances along it
//   Held                              the block of the last visited cell and its slot, so that a chain is walked once per block
//   Residual, residual_test           vk_volume_register_rays' residual test of a measured ray: vk_volume_score_poses' too
// The definitions are in include/vk.h at vk_volume_integrate_rays (the ray, the walk) and vk_volume_register_rays (the residual
// test); vk_volume_carve_rays walks the same cells between other ends. Every float expression keeps the order and grouping
// vk.h gives it.
#pragma once

#include "vk_block_walk.hpp"

namespace vk
{

constexpr int kMaxGuardCells = 1024;         // ceilf(tb - ta) saturates here; tb - ta <= 4 tr <= 256, so it never does

enum { kIntegrated = 0, kNoMeasurement = 1, kInvalid = 2 };

// what every call along range rays carries into its kernels: an operation's parameter block begins with it
struct RangeRays
{
  vk_volume v;
  int total;                    // main + excess entries = pool slots
  int count;
  int voxel_units;
  float r_min, r_max;
  const float* rays;            // [6 * count]
  const float* ranges;          // [count]
  const vk_transform* pose;     // device, or null
};

// The host's checks of the arguments such calls share, and the carry filled from them: VK_OK or VK_ERR_ARGUMENT, nothing is
// enqueued. `allowed` is the mask of the flags the operation knows, `limit` the most rays a call may bring; `walks`: the
// operation walks a band of the truncation length, whose guard holds up to 64 voxels.
inline int range_rays_arguments(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* pose_dev,
    int32_t flags, float r_min, float r_max, const void* workspace, int32_t allowed, int32_t limit, bool pose_may_be_null, bool walks,
    RangeRays& R)
{
  VK_REQUIRE(volume_ok(v) && workspace && (pose_dev || pose_may_be_null));
  VK_REQUIRE((flags & ~allowed) == 0);
  VK_REQUIRE(__builtin_isfinite(r_min) && __builtin_isfinite(r_max) && r_min >= 0.0f && r_min < r_max);
  VK_REQUIRE(count >= 0 && count <= limit);
  VK_REQUIRE((rays && ranges) || count == 0);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);                       // accumulators are zeroed 16 bytes at a time
  VK_REQUIRE(!walks || v->truncation_length / v->voxel_length <= 64.0f);                 // (false for a NaN)
  R.v = *v;
  R.total = v->main_block_count + v->excess_block_count;
  R.count = count;
  R.voxel_units = (flags & VK_RAYS_VOXEL_UNITS) ? 1 : 0;
  R.r_min = r_min;
  R.r_max = r_max;
  R.rays = rays;
  R.ranges = ranges;
  R.pose = pose_dev;
  return VK_OK;
}

// vk_volume_cast_rays' ray (load_ray), and its range
struct RangeRay : Ray
{
  float r;                      // the range in voxels
  int kind;
};

// ray i of the call through `pose`: a valid ray has a measurement iff r_min <= range <= r_max
__device__ __forceinline__ RangeRay load_range_ray(const RangeRays& R, size_t i, const vk_transform* pose)
{
  const bool voxel_units = R.voxel_units != 0;
  RangeRay ray;
  static_cast<Ray&>(ray) = load_ray(R.rays, i, pose, R.v.voxel_length, voxel_units);
  const float range = R.ranges[i];
  ray.r = voxel_units ? range : range / R.v.voxel_length;
  const bool measured = R.r_min <= range && range <= R.r_max;         // false for a NaN
  ray.kind = ray.valid ? (measured ? kIntegrated : kNoMeasurement) : kInvalid;
  return ray;
}

// ray i as the call carries it
__device__ __forceinline__ RangeRay load_range_ray(const RangeRays& R, size_t i) { return load_range_ray(R, i, R.pose); }

// the first crossing of a face along one axis of a lattice of EDGE voxels (1: cells, 8: blocks) and the distance between
// crossings: +infinity for an axis the ray does not move along. (float)(EDGE * k) and (float)EDGE / n are exact for EDGE = 1.
template <int EDGE>
__device__ __forceinline__ void axis_setup(float ta, float p, float n, int c, int& step, float& tmax, float& tdelta)
{
  step = n > 0.0f ? 1 : (n < 0.0f ? -1 : 0);
  tmax = tdelta = INFINITY;
  if (n > 0.0f)
  {
    tmax = ta + ((float)(EDGE * (c + 1)) - p) / n;
    tdelta = (float)EDGE / n;
  }
  else if (n < 0.0f)
  {
    tmax = ta + ((float)(EDGE * c) - p) / n;
    tdelta = (float)EDGE / fabsf(n);
  }
}

// the axis of the smallest of three crossings, x before y before z on a tie (a NaN is never the smaller), and that crossing
__device__ __forceinline__ int least_axis(float mx, float my, float mz, float& least)
{
  int axis = 0;
  least = mx;
  if (my < least) { axis = 1;  least = my; }
  if (mz < least) { axis = 2;  least = mz; }
  return axis;
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
  axis_setup<1>(ta, px, ray.n.x, cx, sx, mx, dx);
  axis_setup<1>(ta, py, ray.n.y, cy, sy, my, dy);
  axis_setup<1>(ta, pz, ray.n.z, cz, sz, mz, dz);
  const int guard = 3 * (vclampi(f2i(ceilf(tb - ta)), 0, kMaxGuardCells) + 2);
  for (int turn = 0; turn < guard; ++turn)
  {
    float least;
    const int axis = least_axis(mx, my, mz, least);
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

// vk_volume_register_rays' residual test of a measured ray (include/vk.h): the trilinear sample at the ray's endpoint `e`
// where the map holds all eight voxels around it (`sampled`), a residual where |D| is inside the band
struct Residual
{
  bool sampled, residual;
  float D, gx, gy, gz;          // the distance and its gradient at e, of a sampled ray
  f3 e;
};

__device__ __forceinline__ Residual residual_test(const vk_volume& v, int total, const RangeRay& ray, float band)
{
  Residual out;
  out.sampled = out.residual = false;
  out.D = out.gx = out.gy = out.gz = 0.0f;
  out.e = f3{ray.o.x + ray.r * ray.n.x, ray.o.y + ray.r * ray.n.y, ray.o.z + ray.r * ray.n.z};
  const Cell cell = read_cell<false, true>(v, total, out.e, finite3(out.e));
  if (cell.all_d)
  {
    out.sampled = true;
    out.D = trilinear_gradient(cell.distance, cell.l.fx, cell.l.fy, cell.l.fz, out.gx, out.gy, out.gz);
    out.residual = fabsf(out.D) < band;
  }
  return out;
}

}  // namespace vk
