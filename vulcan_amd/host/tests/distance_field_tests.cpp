// distance_field_tests.cpp — Volume::DistanceField(grid, options, buffers) and Volume::ClassifyCells through the C++ class layer ->
// C ABI -> HIP kernels (no upstream case: the reference never leaves its truncation band). The calls are held against the CPU
// statement bit for bit by tests/test_gpu_distance_field.py; these cases are what a user of the class sees: in front of a wall
// fused from range rays the clearance is the distance to the wall's plane, an empty volume is unknown and infinitely far from
// anything, and the calls are allowed while a frame is announced. Harness: volume_test_support.h.
//
//   ./distance_field_tests            run everything (needs a GPU)
//   ./distance_field_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

#include <limits>

static const float kWall = 1.0f;                     // a fronto-parallel plane, metres in front of the sensor

struct Field
{
  std::vector<unsigned char> classes;
  std::vector<float> distance;
  std::vector<int> squared_cells;
};

static Field Read(const DistanceFieldBuffers& buffers, bool squared)
{
  Field f;
  f.classes.resize(buffers.classes.GetSize());
  f.distance.resize(buffers.distance.GetSize());
  buffers.classes.CopyToHost(f.classes.data());
  buffers.distance.CopyToHost(f.distance.data());
  if (squared)
  {
    f.squared_cells.resize(buffers.squared_cells.GetSize());
    buffers.squared_cells.CopyToHost(f.squared_cells.data());
  }
  return f;
}

static CellGrid Grid(int ox, int oy, int oz, int nx, int ny, int nz, int stride)
{
  CellGrid g;
  g.origin[0] = ox;  g.origin[1] = oy;  g.origin[2] = oz;
  g.dims[0] = nx;  g.dims[1] = ny;  g.dims[2] = nz;
  g.stride = stride;
  return g;
}

// A cell in front of the wall whose nearest wall point lies inside the fused patch is as far from the nearest occupied cell
// as its centre is from the plane, within one cell diagonal plus one voxel length: sites are quantised to cells, and the first
// occupied voxel lies within a voxel behind the zero crossing. (The CPU statement measures 4.0 mm at stride 1 and 8.0 mm at
// stride 4 on this scene, against bounds of 21.9 and 63.4 mm.)
TEST(DistanceField, ClearanceInFrontOfAWall)
{
  const std::vector<Ray> rays = PixelRays(BumpsFrame(Transform()));
  std::vector<float> ranges;
  for (const Ray& ray : rays) ranges.push_back(kWall * Length(ray.direction));
  Buffer<Ray> rays_dev(rays.size());
  Buffer<float> ranges_dev(ranges.size());
  rays_dev.CopyFromHost(rays.data());
  ranges_dev.CopyFromHost(ranges.data());
  auto volume = Fresh(4093, 2048);
  IntegrateRaysOptions fuse;
  fuse.one_observation = true;
  const IntegrateRaysCounts fused = volume->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size()), nullptr, fuse);
  ASSERT_EQ(int(rays.size()), fused.integrated);
  ASSERT_EQ(0, fused.lost);

  DistanceFieldBuffers buffers;
  // 0.64 x 0.38 m of the wall's middle, from 0.70 m to 1.02 m along the view: the patch reaches 0.58 x 0.44 m either way
  const int strides[2] = {1, 4}, caps[2] = {64, 16};
  for (int s = 0; s < 2; ++s)
  {
    const int stride = strides[s];
    const CellGrid grid = Grid(-40, -24, 88, 80 / stride, 48 / stride, 40 / stride, stride);
    DistanceFieldOptions options;
    options.max_cells = caps[s];
    options.squared = true;
    volume->DistanceField(grid, options, buffers);
    const Field f = Read(buffers, true);
    ASSERT_EQ(grid.Cells(), f.distance.size());
    const float cell = float(stride) * kVoxel;
    const float bound = std::sqrt(3.0f) * cell + kVoxel;
    int checked = 0, occupied = 0, free_cells = 0;
    float worst = 0.0f;
    for (int k = 0; k < grid.dims[2]; ++k)
      for (int j = 0; j < grid.dims[1]; ++j)
        for (int i = 0; i < grid.dims[0]; ++i)
        {
          const size_t at = (size_t(k) * grid.dims[1] + j) * grid.dims[0] + i;
          const unsigned char c = f.classes[at];
          ASSERT_TRUE(c == VK_CELL_UNKNOWN || c == VK_CELL_FREE || c == VK_CELL_OCCUPIED);
          occupied += c == VK_CELL_OCCUPIED;
          free_cells += c == VK_CELL_FREE;
          ASSERT_TRUE((c == VK_CELL_OCCUPIED) == (f.squared_cells[at] == 0));
          ASSERT_TRUE((f.squared_cells[at] == VK_FIELD_BEYOND) == std::isinf(f.distance[at]));
          const float analytic = kWall - (float(grid.origin[2]) + float(stride) * (float(k) + 0.5f)) * kVoxel;
          if (analytic <= 0.0f || c == VK_CELL_OCCUPIED) continue;
          ++checked;
          ASSERT_TRUE(std::isfinite(f.distance[at]));
          worst = std::max(worst, std::fabs(f.distance[at] - analytic));
        }
    std::printf("         stride %d: %d occupied and %d free cells, %d cells in front of the wall within %.4f m of the plane's distance "
        "(bound %.4f m)\n", stride, occupied, free_cells, checked, worst, bound);
    ASSERT_TRUE(occupied > 100 && free_cells > 100 && checked > 1000);
    ASSERT_TRUE(worst <= bound);

    // the class grid alone is the field's
    Buffer<unsigned char> classes;
    volume->ClassifyCells(grid, options.occupied_below, classes);
    std::vector<unsigned char> alone(classes.GetSize());
    classes.CopyToHost(alone.data());
    ASSERT_TRUE(alone == f.classes);
  }

  // signed: negative exactly on the occupied cells
  DistanceFieldOptions with_sign;
  with_sign.max_cells = 16;
  with_sign.is_signed = true;
  volume->DistanceField(Grid(-40, -24, 88, 20, 12, 10, 4), with_sign, buffers);
  const Field f = Read(buffers, false);
  for (size_t at = 0; at < f.distance.size(); ++at) ASSERT_TRUE((f.distance[at] < 0.0f) == (f.classes[at] == VK_CELL_OCCUPIED));

  // what the C ABI refuses arrives as an exception
  ASSERT_THROW(volume->DistanceField(Grid(-40, -24, 88, 20, 12, 10, 3), DistanceFieldOptions(), buffers));
  ASSERT_THROW(volume->DistanceField(Grid(-38, -24, 88, 20, 12, 10, 4), DistanceFieldOptions(), buffers));
  ASSERT_THROW(volume->DistanceField(Grid(0, 0, 0, 0, 12, 10, 1), DistanceFieldOptions(), buffers));
  DistanceFieldOptions bad;
  bad.max_cells = 257;
  ASSERT_THROW(volume->DistanceField(Grid(0, 0, 0, 8, 8, 8, 1), bad, buffers));
  bad = DistanceFieldOptions();
  bad.site_mask = 0;
  ASSERT_THROW(volume->DistanceField(Grid(0, 0, 0, 8, 8, 8, 1), bad, buffers));
  Buffer<unsigned char> classes;
  ASSERT_THROW(volume->ClassifyCells(Grid(0, 0, 0, 8, 8, 8, 1), std::numeric_limits<float>::quiet_NaN(), classes));
}

TEST(DistanceField, AnEmptyVolumeIsUnknownAndFarFromAnything)
{
  auto volume = Fresh(509, 64);
  DistanceFieldBuffers buffers;
  DistanceFieldOptions options;
  options.squared = true;
  const CellGrid grid = Grid(-64, -32, 0, 70, 33, 65, 2);
  volume->DistanceField(grid, options, buffers);
  const Field f = Read(buffers, true);
  ASSERT_EQ(grid.Cells(), f.classes.size());
  for (size_t at = 0; at < f.classes.size(); ++at)
  {
    ASSERT_EQ(int(VK_CELL_UNKNOWN), int(f.classes[at]));
    ASSERT_TRUE(f.squared_cells[at] == VK_FIELD_BEYOND);
    ASSERT_TRUE(std::isinf(f.distance[at]) && f.distance[at] > 0.0f);
  }
  ASSERT_EQ(0, volume->GetAllocatedBlockCount());
}

// the calls only read: they are allowed while Tracer::Trace(keyframe, next_frame) has the next frame's requests in the volume,
// and what was made ahead stays valid
TEST(DistanceField, AllowedWhileAFrameIsAnnounced)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  DistanceFieldBuffers before, during;
  const CellGrid grid = Grid(-48, -32, 96, 48, 32, 40, 2);
  DistanceFieldOptions options;
  options.max_cells = 24;
  volume->DistanceField(grid, options, before);
  const Field was = Read(before, false);
  int occupied = 0;
  for (unsigned char c : was.classes) occupied += c == VK_CELL_OCCUPIED;
  ASSERT_TRUE(occupied > 100);

  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = BumpsFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const std::vector<vk_voxel> voxels = Voxels(*volume);
  volume->DistanceField(grid, options, during);
  Buffer<unsigned char> classes;
  volume->ClassifyCells(grid, options.occupied_below, classes);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const Field now = Read(during, false);
  ASSERT_TRUE(now.classes == was.classes);
  ASSERT_TRUE(std::memcmp(now.distance.data(), was.distance.data(), was.distance.size() * sizeof(float)) == 0);
  const std::vector<vk_voxel> after = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(voxels.data(), after.data(), voxels.size() * sizeof(vk_voxel)) == 0);
  volume->CancelRequestsAhead(3);
}

int main(int argc, char** argv) { return RunTests("distance_field_tests", argc, argv); }
