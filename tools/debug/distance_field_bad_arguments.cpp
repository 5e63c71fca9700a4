// distance_field_bad_arguments.cpp — every refusal of the host checks of vk_volume_classify_cells, vk_grid_distance_transform,
// vk_volume_distance_field and their two workspace sizes (include/vk.h), with addresses that are no memory: a stand-alone
// program for a host sanitizer run of those checks. No GPU is needed or touched: each call has to return VK_ERR_ARGUMENT
// before anything is enqueued. Build it with the entry points' own source, the rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc -I tools/debug vulcan_amd/csrc/vk_distance_field.hip tools/debug/distance_field_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o distance_field_bad_arguments
#include "bad_arguments.h"

static vk_cell_grid Grid(int ox = 0, int oy = 0, int oz = 0, int nx = 8, int ny = 8, int nz = 8, int stride = 1)
{
  vk_cell_grid g = {};
  g.origin[0] = ox;  g.origin[1] = oy;  g.origin[2] = oz;
  g.dims[0] = nx;  g.dims[1] = ny;  g.dims[2] = nz;
  g.stride = stride;
  return g;
}

static vk_distance_field_params Params(int flags = 0, int site_mask = VK_CELL_OCCUPIED, int max_cells = 16, float occupied_below = 0.0f)
{
  vk_distance_field_params p = {};
  p.flags = flags;
  p.site_mask = site_mask;
  p.max_cells = max_cells;
  p.occupied_below = occupied_below;
  return p;
}

static int32_t* const kOddInts = reinterpret_cast<int32_t*>(uintptr_t(12288 + 2));
static float* const kOddFloats = reinterpret_cast<float*>(uintptr_t(8192 + 2));
static void* const kOddWorkspace = reinterpret_cast<void*>(uintptr_t(16384 + 8));

static int Classify(const vk_volume* v, const vk_cell_grid* g, float occupied_below = 0.0f, uint8_t* classes = kBytes)
{
  return vk_volume_classify_cells(v, g, occupied_below, classes, nullptr);
}

static int Transform(const uint8_t* classes, const int32_t* dims, int site_mask = 4, int max_cells = 16, int32_t* d2 = kInts,
    void* workspace = kWorkspace)
{
  return vk_grid_distance_transform(classes, dims, site_mask, max_cells, d2, workspace, nullptr);
}

static int Field(const vk_volume* v, const vk_cell_grid* g, const vk_distance_field_params* p, uint8_t* classes = kBytes,
    int32_t* d2 = kInts, float* distance = kFloats, void* workspace = kWorkspace)
{
  return vk_volume_distance_field(v, g, p, classes, d2, distance, workspace, nullptr);
}

int main()
{
  static_assert(sizeof(vk_cell_grid) == 32 && sizeof(vk_distance_field_params) == 16, "vk.h's sizes");
  const vk_volume v = Volume();
  const vk_cell_grid g = Grid();
  const vk_distance_field_params p = Params();
  const int32_t dims[3] = {8, 8, 8};

  // a null pointer that is not optional
  EXPECT(VK_ERR_ARGUMENT, Classify(nullptr, &g));
  EXPECT(VK_ERR_ARGUMENT, Classify(&v, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Classify(&v, &g, 0.0f, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Transform(nullptr, dims));
  EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, dims, 4, 16, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, dims, 4, 16, kInts, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Field(nullptr, &g, &p));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, nullptr, &p));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &p, kBytes, kInts, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &p, kBytes, kInts, kFloats, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &p, nullptr, nullptr, nullptr));

  // a volume vk_volume_sample would refuse
  {
    vk_volume broken = Volume();
    broken.hash_entries = nullptr;
    EXPECT(VK_ERR_ARGUMENT, Classify(&broken, &g));
    EXPECT(VK_ERR_ARGUMENT, Field(&broken, &g, &p));
    broken = Volume();
    broken.voxel_length = 0.0f;
    EXPECT(VK_ERR_ARGUMENT, Classify(&broken, &g));
    EXPECT(VK_ERR_ARGUMENT, Field(&broken, &g, &p));
    broken = Volume();
    broken.main_block_count = 0;
    EXPECT(VK_ERR_ARGUMENT, Classify(&broken, &g));
    EXPECT(VK_ERR_ARGUMENT, Field(&broken, &g, &p));
    broken = Volume();
    broken.excess_block_count = kMost;
    EXPECT(VK_ERR_ARGUMENT, Classify(&broken, &g));
    EXPECT(VK_ERR_ARGUMENT, Field(&broken, &g, &p));
    broken = Volume((uintptr_t(1) << 20) + 8);           // buffers that are not aligned
    EXPECT(VK_ERR_ARGUMENT, Classify(&broken, &g));
    EXPECT(VK_ERR_ARGUMENT, Field(&broken, &g, &p));
  }

  // the grid: stride, alignment of the origin, its range, the dims and the cell count
  const vk_cell_grid bad_grids[] = {Grid(0, 0, 0, 8, 8, 8, 0), Grid(0, 0, 0, 8, 8, 8, 3), Grid(0, 0, 0, 8, 8, 8, 6), Grid(0, 0, 0, 8, 8, 8, 16),
      Grid(0, 0, 0, 8, 8, 8, -1), Grid(0, 0, 0, 8, 8, 8, -2), Grid(0, 0, 0, 8, 8, 8, kMost), Grid(0, 0, 0, 8, 8, 8, kLeast),
      Grid(1, 0, 0, 8, 8, 8, 2), Grid(0, 2, 0, 8, 8, 8, 4), Grid(0, 0, 4, 8, 8, 8, 8), Grid(-3, 0, 0, 8, 8, 8, 2),
      Grid((1 << 20) + 1, 0, 0), Grid(0, -(1 << 20) - 1, 0), Grid(0, 0, kMost), Grid(kLeast, 0, 0), Grid(0, (1 << 20) + 8, 0, 8, 8, 8, 8),
      Grid(0, 0, 0, 0, 8, 8), Grid(0, 0, 0, 8, -1, 8), Grid(0, 0, 0, 8, 8, 1025), Grid(0, 0, 0, kMost, 1, 1), Grid(0, 0, 0, 1, kLeast, 1),
      Grid(0, 0, 0, 1024, 1024, 129), Grid(0, 0, 0, 1024, 1024, 1024)};
  for (const vk_cell_grid& bad : bad_grids)
  {
    EXPECT(VK_ERR_ARGUMENT, Classify(&v, &bad));
    EXPECT(VK_ERR_ARGUMENT, Field(&v, &bad, &p));
    EXPECT(0, vk_volume_distance_field_workspace_bytes(&bad, &p) != 0);
  }
  const int32_t bad_dims[][3] = {{0, 8, 8}, {8, -1, 8}, {8, 8, 1025}, {kMost, 1, 1}, {1, kLeast, 1}, {1024, 1024, 129}, {1024, 1024, 1024}};
  for (const auto& bad : bad_dims)
  {
    EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, bad));
    EXPECT(0, vk_grid_distance_transform_workspace_bytes(bad) != 0);
  }
  EXPECT(0, vk_grid_distance_transform_workspace_bytes(nullptr) != 0);
  EXPECT(0, vk_volume_distance_field_workspace_bytes(nullptr, &p) != 0);
  EXPECT(0, vk_volume_distance_field_workspace_bytes(&g, nullptr) != 0);

  // the parameters
  const int32_t bad_masks[] = {0, 8, -1, 1 << 16, kMost, kLeast};
  for (int32_t mask : bad_masks)
  {
    const vk_distance_field_params bad = Params(0, mask);
    EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &bad));
    EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, dims, mask));
    EXPECT(0, vk_volume_distance_field_workspace_bytes(&g, &bad) != 0);
  }
  const int32_t bad_caps[] = {0, -1, 257, kMost, kLeast};
  for (int32_t cap : bad_caps)
  {
    const vk_distance_field_params bad = Params(0, 4, cap);
    EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &bad));
    EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, dims, 4, cap));
    EXPECT(0, vk_volume_distance_field_workspace_bytes(&g, &bad) != 0);
  }
  const int32_t bad_flags[] = {2, 3, 4, -1, 1 << 16, kLeast};
  for (int32_t flags : bad_flags)
  {
    const vk_distance_field_params bad = Params(flags);
    EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &bad));
    EXPECT(0, vk_volume_distance_field_workspace_bytes(&g, &bad) != 0);
  }
  const float bad_thresholds[] = {kNan, kInf, -kInf, 1.5f, -1.0001f};
  for (float threshold : bad_thresholds)
  {
    const vk_distance_field_params bad = Params(0, 4, 16, threshold);
    EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &bad));
    EXPECT(VK_ERR_ARGUMENT, Classify(&v, &g, threshold));
    EXPECT(0, vk_volume_distance_field_workspace_bytes(&g, &bad) != 0);
  }

  // alignment: d2 and distance to 4 bytes, the workspace to 16
  EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, dims, 4, 16, kOddInts));
  EXPECT(VK_ERR_ARGUMENT, Transform(kBytes, dims, 4, 16, kInts, kOddWorkspace));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &p, kBytes, kOddInts));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &p, kBytes, kInts, kOddFloats));
  EXPECT(VK_ERR_ARGUMENT, Field(&v, &g, &p, kBytes, kInts, kFloats, kOddWorkspace));

  // the sizes: seven bytes per cell and two flags per 64 cells of a row in 256-byte parts, the same for both calls, at the limits too
  const int32_t largest[3] = {1024, 1024, 128};
  const vk_cell_grid widest = Grid(1 << 20, -(1 << 20), 0, 1024, 1024, 128, 8);
  const vk_distance_field_params most = Params(VK_FIELD_SIGNED, 7, 256, -1.0f);
  EXPECT(1, vk_grid_distance_transform_workspace_bytes(largest) >= (size_t(7) << 27));
  EXPECT(1, vk_volume_distance_field_workspace_bytes(&widest, &most) == vk_grid_distance_transform_workspace_bytes(largest));
  EXPECT(1, vk_grid_distance_transform_workspace_bytes(dims) == 512 * 7 + 2 * 256);   // and two parts of flags
  return Finish("distance_field_bad_arguments");
}
