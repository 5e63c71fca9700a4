// vk_distance_field.hip — the clearance field of a voxel-hashed volume, for gfx950: the volume classified into a dense grid
// of cells (unknown, free, occupied) and the exact Euclidean distance transform of that grid, in integers (no upstream
// counterpart: the reference never leaves its truncation band; ref: src/volume.cu:168-191 for the chain walk. The definition
// is in include/vk.h at vk_volume_distance_field; tests/distance_field_reference.py states it on the CPU and the device is
// held to it bit for bit).
//
// Shape: plain launches on the caller's stream, nothing read back, no atomic, no workgroup waits on another.
//   fill_kernel        the grid becomes VK_CELL_UNKNOWN, 16 bytes per lane
//   classify_kernel    one wave per table entry: an entry that the chain walk finds for its own origin and whose block meets
//                      the grid reads the block's 512 distances and weights (lane = 8 y + x, eight z per lane), folds the
//                      stride^3 groups with wave shuffles and stores the block's cells. A cell has one owner block.
//   x_pass_kernel      one wave per grid row: the row's sites as 64-bit ballots in LDS, a cell's nearest site to either side
//                      by count-leading / count-trailing zeros over the few words within max_cells; writes |dx| as uint16,
//                      and one flag byte per 64 cells: whether any of them found a site
//   axis_pass_kernel   y, then z. A wave owns a tile of 64 cells along x by kRows along the axis and streams the input rows
//                      within max_cells of it: every global access is contiguous along x, nothing is transposed, and the
//                      tile's running minima are registers. It reads the flags of its window's rows first, 64 at a time,
//                      and then only the rows in which one of its 64 cells holds a value (wave-uniform; kAhead loads in
//                      flight): a planner's grid is mostly far from any site, and there a tile costs its flags. What exceeds
//                      max_cells^2 leaves a pass as "none": it could only grow. The y pass writes the flags of its output
//                      for the z pass; the z pass writes d2, the floats, or both.
#include "vk_block_walk.hpp"

using namespace vk;

namespace
{

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRows = 16;                    // cells along the axis in one wave's tile of an axis pass
constexpr int kAhead = 8;                    // input rows an axis pass asks for before it uses the first
constexpr int kNone = 1 << 29;               // no site within reach; + 272^2 stays an int
constexpr int kNoneX = 0xffff;               // the same in the x pass's uint16
constexpr int kMaxDim = 1024, kMaxCellsLog2 = 27, kMaxOrigin = 1 << 20, kMaxReach = 256;
constexpr int kRowWords = kMaxDim / kWave;   // ballots of one row

struct Grid
{
  int ox, oy, oz;
  int nx, ny, nz;
  int shift;                                 // log2(stride)
};

// ---- classify ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void fill_kernel(uint8_t* classes, size_t count)
{
  // the bytes in front of the first 16-byte boundary belong to thread 0, chunk t of the rest to thread t
  const size_t head = ((size_t)0 - reinterpret_cast<uintptr_t>(classes)) & 15;
  const size_t lead = head < count ? head : count;
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (t == 0)
    for (size_t i = 0; i < lead; ++i) classes[i] = (uint8_t)VK_CELL_UNKNOWN;
  const size_t at = lead + t * 16;
  if (at >= count) return;
  if (at + 16 <= count)
  {
    const uint32_t w = 0x01010101u * (uint32_t)VK_CELL_UNKNOWN;
    *reinterpret_cast<uint4*>(classes + at) = make_uint4(w, w, w, w);
  }
  else
    for (size_t i = at; i < count; ++i) classes[i] = (uint8_t)VK_CELL_UNKNOWN;
}

struct ClassifyParams
{
  vk_volume v;
  int total;
  Grid g;
  float occupied_below;
  uint8_t* classes;
};

__global__ __launch_bounds__(kThreads) void classify_kernel(ClassifyParams P)
{
  const int index = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);      // wave-uniform
  if (index >= P.total) return;
  const Entry entry = load_entry(P.v.hash_entries, (uint32_t)index);
  if (entry.data < 0 || entry.data >= P.total) return;
  const Grid& g = P.g;
  const int stride = 1 << g.shift;
  // the block's first voxel relative to the grid's: a multiple of the stride
  const int rx = 8 * entry.ox - g.ox, ry = 8 * entry.oy - g.oy, rz = 8 * entry.oz - g.oz;
  if (rx <= -8 || ry <= -8 || rz <= -8 || rx >= g.nx * stride || ry >= g.ny * stride || rz >= g.nz * stride) return;
  // the entry is the block of its origin only if the chain walk finds it there
  int slot;
  Entry main_entry;
  if (find_block(P.v, P.total, entry.ox, entry.oy, entry.oz, slot, main_entry) != index) return;

  const int lane = lane_id();
  const int x = lane & 7, y = lane >> 3;
  const uint32_t* pool = reinterpret_cast<const uint32_t*>(P.v.voxels) + (size_t)slot * VK_BLOCK_VOXELS * kVoxelWords;
  // two bits per z: observed, occupied
  uint32_t bits = 0u;
#pragma unroll
  for (int z = 0; z < 8; ++z)
  {
    const uint32_t* voxel = pool + (size_t)(z * 64 + lane) * kVoxelWords;
    const float distance = __uint_as_float(voxel[0]);
    const bool observed = (voxel[4] & 0xffffu) != 0u;
    const bool occupied = observed && distance <= P.occupied_below;
    bits |= ((observed ? 1u : 0u) | (occupied ? 2u : 0u)) << (2 * z);
  }
  // fold the cell's voxels along x and y over the lanes, along z in the word
  for (int d = 1; d < stride; d <<= 1)
  {
    bits |= (uint32_t)__shfl_xor((int)bits, d);
    bits |= (uint32_t)__shfl_xor((int)bits, 8 * d);
  }
  for (int d = 1; d < stride; d <<= 1) bits |= bits >> (2 * d);
  if ((x & (stride - 1)) != 0 || (y & (stride - 1)) != 0) return;
  const int vx = rx + x, vy = ry + y;
  if (vx < 0 || vy < 0) return;
  const int i = vx >> g.shift, j = vy >> g.shift;
  if (i >= g.nx || j >= g.ny) return;
  for (int z = 0; z < 8; z += stride)
  {
    const int vz = rz + z;
    if (vz < 0) continue;
    const int k = vz >> g.shift;
    if (k >= g.nz) continue;
    const uint32_t cell = (bits >> (2 * z)) & 3u;
    const int cls = (cell & 2u) ? VK_CELL_OCCUPIED : (cell & 1u) ? VK_CELL_FREE : VK_CELL_UNKNOWN;
    P.classes[((size_t)k * g.ny + j) * g.nx + i] = (uint8_t)cls;
  }
}

// ---- transform --------------------------------------------------------------------------------------------------------

struct RowParams
{
  const uint8_t* classes;
  uint16_t* out;               // |dx| to the nearest site of the row within max_cells, kNoneX without
  uint8_t* flags;              // per row and 64 cells of it: whether one of them has a site within max_cells
  int nx;
  size_t rows;                 // ny * nz
  int site_mask, max_cells;
};

__global__ __launch_bounds__(kThreads) void x_pass_kernel(RowParams P)
{
  __shared__ uint64_t words[kWaves][kRowWords];
  const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
  const size_t row = (size_t)blockIdx.x * kWaves + wave;
  if (row >= P.rows) return;
  uint64_t* mine = words[wave];
  const int chunks = (P.nx + kWave - 1) / kWave;
  const uint8_t* in = P.classes + row * P.nx;
  for (int c = 0; c < chunks; ++c)
  {
    const int i = c * kWave + lane;
    const bool site = i < P.nx && (in[i] & P.site_mask) != 0;
    const uint64_t m = __ballot(site);
    if (lane == 0) mine[c] = m;
  }
  wave_lds_fence();
  const int reach = (P.max_cells + kWave - 1) / kWave;          // words to either side that can hold the nearest site
  uint16_t* out = P.out + row * P.nx;
  for (int c = 0; c < chunks; ++c)
  {
    int right = kNone, left = kNone;
    // from the farthest word inwards, so that the nearest wins
    for (int w = reach; w >= 0; --w)
    {
      uint64_t m = c + w < chunks ? mine[c + w] : 0ull;
      uint64_t n = c - w >= 0 ? mine[c - w] : 0ull;
      if (w == 0)
      {
        m &= ~0ull << lane;
        n &= (2ull << lane) - 1ull;
      }
      if (m) right = kWave * w + (__ffsll((unsigned long long)m) - 1) - lane;
      if (n) left = lane + kWave * w - (63 - __clzll((long long)n));
    }
    const int dx = vmini(left, right);
    const int i = c * kWave + lane;
    const bool within = i < P.nx && dx <= P.max_cells;
    if (i < P.nx) out[i] = (uint16_t)(within ? dx : kNoneX);
    const bool any = __any(within);
    if (lane == 0) P.flags[row * chunks + c] = any ? 1 : 0;
  }
}

struct AxisParams
{
  const void* in;              // FIRST: the x pass's uint16; else int32 squared distances, kNone without
  int32_t* out;                // !LAST: int32, kNone without. LAST: d2 (VK_FIELD_BEYOND without), or null
  float* distance;             // LAST: the float field, or null
  const uint8_t* in_flags;     // per element of a line and 64 cells along x: whether `in` holds a value there
  uint8_t* out_flags;          // !LAST: the same of `out`
  size_t flag_step;            // flags between neighbours along the axis
  size_t flag_other_step;      // flags between neighbours along the third axis (blockIdx.z)
  const uint8_t* classes;      // LAST with a sign: only site cells are written, negated
  int site_mask;               // 0: every cell is written
  int nx;
  int length;                  // cells along the axis
  size_t step;                 // elements between neighbours along the axis
  size_t other_step;           // elements between neighbours along the third axis (blockIdx.z)
  int max_cells;
  float cell_voxels, voxel_length;
};

template <bool FIRST>
__device__ __forceinline__ int load_row(const AxisParams& P, size_t at)
{
  if (FIRST)
  {
    const int dx = (int)static_cast<const uint16_t*>(P.in)[at];
    return dx == kNoneX ? kNone : dx * dx;
  }
  return static_cast<const int32_t*>(P.in)[at];
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kThreads) void axis_pass_kernel(AxisParams P)
{
  const int lane = lane_id();
  const int x = (int)blockIdx.x * kWave + lane;
  const int first = ((int)blockIdx.y * kWaves + (int)(threadIdx.x >> 6)) * kRows;     // wave-uniform
  if (first >= P.length) return;
  const bool active = x < P.nx;
  const size_t base = (size_t)blockIdx.z * P.other_step + (size_t)(active ? x : 0);
  const size_t flag_base = (size_t)blockIdx.z * P.flag_other_step + blockIdx.x;
  const int lo = vmaxi(0, first - P.max_cells), hi = vmini(P.length - 1, first + kRows - 1 + P.max_cells);
  int best[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) best[r] = kNone;
  // the window's rows, 64 flags at a time: only a row in which one of the tile's 64 cells holds a value is read
  for (int a = lo; a <= hi; a += kWave)
  {
    const int mine = a + lane;
    uint64_t rows = __ballot(mine <= hi && P.in_flags[flag_base + (size_t)(mine <= hi ? mine : hi) * P.flag_step] != 0);
    while (rows)
    {
      int row[kAhead], v[kAhead];
#pragma unroll
      for (int b = 0; b < kAhead; ++b)
      {
        row[b] = rows ? a + (__ffsll((unsigned long long)rows) - 1) : -1;
        rows &= rows - 1ull;
      }
#pragma unroll
      for (int b = 0; b < kAhead; ++b) v[b] = (active && row[b] >= 0) ? load_row<FIRST>(P, base + (size_t)row[b] * P.step) : kNone;
#pragma unroll
      for (int b = 0; b < kAhead; ++b)
      {
        if (row[b] < 0) continue;
        const int d = first - row[b];
#pragma unroll
        for (int r = 0; r < kRows; ++r) best[r] = vmini(best[r], v[b] + (d + r) * (d + r));
      }
    }
  }
  const int cap = P.max_cells * P.max_cells;
#pragma unroll
  for (int r = 0; r < kRows; ++r)
  {
    if (first + r >= P.length) break;
    const size_t at = base + (size_t)(first + r) * P.step;
    const bool beyond = best[r] > cap;
    if (!LAST)
    {
      const bool any = __any(active && !beyond);
      if (lane == 0) P.out_flags[flag_base + (size_t)(first + r) * P.flag_step] = any ? 1 : 0;
      if (active) P.out[at] = beyond ? kNone : best[r];
      continue;
    }
    if (!active) continue;
    if (P.site_mask)
    {
      if ((P.classes[at] & P.site_mask) == 0) continue;
      P.distance[at] = beyond ? -INFINITY : -((sqrtf((float)best[r]) * P.cell_voxels) * P.voxel_length);
      continue;
    }
    if (P.out) P.out[at] = beyond ? VK_FIELD_BEYOND : best[r];
    if (P.distance) P.distance[at] = beyond ? INFINITY : (sqrtf((float)best[r]) * P.cell_voxels) * P.voxel_length;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

bool dims_ok(const int32_t* dims)
{
  if (!dims) return false;
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 1 || dims[a] > kMaxDim) return false;
  return (int64_t)dims[0] * dims[1] * dims[2] <= ((int64_t)1 << kMaxCellsLog2);
}

bool grid_ok(const vk_cell_grid* grid)
{
  if (!grid || !dims_ok(grid->dims)) return false;
  if (grid->stride != 1 && grid->stride != 2 && grid->stride != 4 && grid->stride != 8) return false;
  for (int a = 0; a < 3; ++a)
    if (grid->origin[a] < -kMaxOrigin || grid->origin[a] > kMaxOrigin || (grid->origin[a] & (grid->stride - 1)) != 0) return false;
  return true;
}

bool threshold_ok(float occupied_below) { return isfinite(occupied_below) && occupied_below >= -1.0f && occupied_below <= 1.0f; }

bool params_ok(const vk_distance_field_params* p)
{
  return p && (p->flags & ~VK_FIELD_SIGNED) == 0 && p->site_mask >= 1 && p->site_mask <= 7 && p->max_cells >= 1 &&
         p->max_cells <= kMaxReach && threshold_ok(p->occupied_below);
}

size_t cell_count(const int32_t* dims) { return (size_t)dims[0] * dims[1] * dims[2]; }

// the workspace: the x pass's uint16 grid, the y pass's int32 grid, a class grid for a caller who wants none, and the two
// passes' flags, one byte per grid row and 64 cells of it
size_t flag_count(const int32_t* dims) { return (size_t)((dims[0] + kWave - 1) / kWave) * dims[1] * dims[2]; }
size_t squares_offset(const int32_t* dims) { return align_up(cell_count(dims) * sizeof(uint16_t)); }
size_t classes_offset(const int32_t* dims) { return squares_offset(dims) + align_up(cell_count(dims) * sizeof(int32_t)); }
size_t flags_offset(const int32_t* dims) { return classes_offset(dims) + align_up(cell_count(dims)); }
size_t workspace_bytes(const int32_t* dims) { return flags_offset(dims) + 2 * align_up(flag_count(dims)); }

int classify(const vk_volume* v, const vk_cell_grid* grid, float occupied_below, uint8_t* classes, hipStream_t s)
{
  const size_t cells = cell_count(grid->dims);
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((cells / 16 + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, classes, cells);
  VK_LAUNCH_CHECK();
  ClassifyParams P;
  P.v = *v;
  P.total = v->main_block_count + v->excess_block_count;
  P.g.ox = grid->origin[0];  P.g.oy = grid->origin[1];  P.g.oz = grid->origin[2];
  P.g.nx = grid->dims[0];  P.g.ny = grid->dims[1];  P.g.nz = grid->dims[2];
  P.g.shift = grid->stride == 1 ? 0 : grid->stride == 2 ? 1 : grid->stride == 4 ? 2 : 3;
  P.occupied_below = occupied_below;
  P.classes = classes;
  hipLaunchKernelGGL(classify_kernel, dim3((unsigned)(((size_t)P.total + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, P);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

// classes -> d2 and/or the floats. With `negate` the last pass writes only the cells of classes & negate, negated.
int transform(const uint8_t* classes, const int32_t* dims, int site_mask, int max_cells, int32_t* d2, float* distance, int negate,
    float cell_voxels, float voxel_length, void* workspace, hipStream_t s)
{
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint16_t* rows = reinterpret_cast<uint16_t*>(ws);
  int32_t* squares = reinterpret_cast<int32_t*>(ws + squares_offset(dims));
  uint8_t* row_flags = ws + flags_offset(dims);
  uint8_t* square_flags = row_flags + align_up(flag_count(dims));
  const size_t chunks = (size_t)((nx + kWave - 1) / kWave);

  RowParams R;
  R.classes = classes;
  R.out = rows;
  R.flags = row_flags;
  R.nx = nx;
  R.rows = (size_t)ny * nz;
  R.site_mask = site_mask;
  R.max_cells = max_cells;
  hipLaunchKernelGGL(x_pass_kernel, dim3((unsigned)((R.rows + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, R);
  VK_LAUNCH_CHECK();

  const int tile = kWaves * kRows;
  AxisParams A;
  A.in = rows;
  A.out = squares;
  A.distance = nullptr;
  A.in_flags = row_flags;
  A.out_flags = square_flags;
  A.flag_step = chunks;
  A.flag_other_step = chunks * ny;
  A.classes = nullptr;
  A.site_mask = 0;
  A.nx = nx;
  A.length = ny;
  A.step = (size_t)nx;
  A.other_step = (size_t)nx * ny;
  A.max_cells = max_cells;
  A.cell_voxels = cell_voxels;
  A.voxel_length = voxel_length;
  hipLaunchKernelGGL((axis_pass_kernel<true, false>), dim3((unsigned)((nx + kWave - 1) / kWave), (unsigned)((ny + tile - 1) / tile), (unsigned)nz),
      dim3(kThreads), 0, s, A);
  VK_LAUNCH_CHECK();

  A.in = squares;
  A.out = d2;
  A.in_flags = square_flags;
  A.out_flags = nullptr;
  A.flag_step = chunks * ny;
  A.flag_other_step = chunks;
  A.distance = distance;
  A.classes = classes;
  A.site_mask = negate;
  A.length = nz;
  A.step = (size_t)nx * ny;
  A.other_step = (size_t)nx;
  hipLaunchKernelGGL((axis_pass_kernel<false, true>), dim3((unsigned)((nx + kWave - 1) / kWave), (unsigned)((nz + tile - 1) / tile), (unsigned)ny),
      dim3(kThreads), 0, s, A);
  VK_LAUNCH_CHECK();
  return VK_OK;
}

}  // namespace

extern "C" {

int vk_volume_classify_cells(const vk_volume* v, const vk_cell_grid* grid, float occupied_below, uint8_t* classes, void* stream)
{
  VK_REQUIRE(v && grid && classes);
  VK_REQUIRE(volume_ok(v));
  VK_REQUIRE(grid_ok(grid));
  VK_REQUIRE(threshold_ok(occupied_below));
  return classify(v, grid, occupied_below, classes, vk_s(stream));
}

size_t vk_grid_distance_transform_workspace_bytes(const int32_t dims[3])
{
  return dims_ok(dims) ? workspace_bytes(dims) : 0;
}

int vk_grid_distance_transform(const uint8_t* classes, const int32_t dims[3], int32_t site_mask, int32_t max_cells, int32_t* d2,
    void* workspace, void* stream)
{
  VK_REQUIRE(classes && dims && d2 && workspace);
  VK_REQUIRE(dims_ok(dims));
  VK_REQUIRE(site_mask >= 1 && site_mask <= 7);
  VK_REQUIRE(max_cells >= 1 && max_cells <= kMaxReach);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(d2) & 3) == 0);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  return transform(classes, dims, site_mask, max_cells, d2, nullptr, 0, 0.0f, 0.0f, workspace, vk_s(stream));
}

size_t vk_volume_distance_field_workspace_bytes(const vk_cell_grid* grid, const vk_distance_field_params* p)
{
  return grid_ok(grid) && params_ok(p) ? workspace_bytes(grid->dims) : 0;
}

int vk_volume_distance_field(const vk_volume* v, const vk_cell_grid* grid, const vk_distance_field_params* p, uint8_t* classes,
    int32_t* d2, float* distance, void* workspace, void* stream)
{
  VK_REQUIRE(v && grid && p && distance && workspace);
  VK_REQUIRE(volume_ok(v));
  VK_REQUIRE(grid_ok(grid));
  VK_REQUIRE(params_ok(p));
  VK_REQUIRE((reinterpret_cast<uintptr_t>(d2) & 3) == 0);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(distance) & 3) == 0);
  VK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  hipStream_t s = vk_s(stream);
  if (!classes) classes = static_cast<uint8_t*>(workspace) + classes_offset(grid->dims);
  int e = classify(v, grid, p->occupied_below, classes, s);
  if (e != VK_OK) return e;
  const float cell_voxels = (float)grid->stride;
  e = transform(classes, grid->dims, p->site_mask, p->max_cells, d2, distance, 0, cell_voxels, v->voxel_length, workspace, s);
  if (e != VK_OK) return e;
  // the sign: the site cells take the negated distance to the nearest cell that is no site
  if (p->flags & VK_FIELD_SIGNED)
    e = transform(classes, grid->dims, 7 ^ p->site_mask, p->max_cells, nullptr, distance, p->site_mask, cell_voxels, v->voxel_length,
        workspace, s);
  return e;
}

}  // extern "C"
