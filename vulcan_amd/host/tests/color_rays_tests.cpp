// color_rays_tests.cpp — Volume::ColorRays(rays, ranges, colors, count, pose, options) through the C++ class layer -> C ABI ->
// HIP kernels (no upstream case: the reference colours only from the pixels of one pinhole image). The call is held against
// the CPU statement bit for bit by tests/test_gpu_color_rays.py; these cases are what a user of the class sees: a map built
// from range rays alone, coloured from the same rays, shows those colours to CastRays and to the mesh; a volume with an
// announced frame refuses; no rays are no call. Harness: volume_test_support.h.
//
//   ./color_rays_tests            run everything (needs a GPU)
//   ./color_rays_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// the largest channel of |colour - paint| at the new hit and at a vertex of the mesh, tests/test_color_rays_reference.py:
// twice the maxima the statement measures in its scenario
static const float kCastBound = 2 * 0.0130f, kMeshBound = 2 * 0.0158f;

// the colour of a point of the volume's frame, in metres: a smooth function
static Vector3f Paint(const Vector3f& p)
{
  return Vector3f(float(0.5 + 0.4 * std::sin(6.0 * p[0])), float(0.5 + 0.4 * std::sin(6.0 * p[1] + 1.0)),
      float(0.5 + 0.4 * std::sin(6.0 * (double(p[0]) + p[1]) + 2.0)));
}

static Vector3f Along(const Ray& ray, float t)
{
  const float length = Length(ray.direction);
  return Vector3f(ray.origin[0] + t * ray.direction[0] / length, ray.origin[1] + t * ray.direction[1] / length,
      ray.origin[2] + t * ray.direction[2] / length);
}

static float Difference(const float* color, const Vector3f& paint)
{
  return std::max(std::fabs(color[0] - paint[0]), std::max(std::fabs(color[1] - paint[1]), std::fabs(color[2] - paint[2])));
}

struct Hits
{
  std::vector<float> t;
  std::vector<int> status;
  std::vector<vk_voxel> samples;
};

static Hits Cast(const Volume& volume, const Buffer<Ray>& rays_dev)
{
  const size_t n = rays_dev.GetSize();
  Buffer<float> t_dev(n);
  Buffer<int> status_dev(n);
  Buffer<Voxel> samples_dev(n);
  volume.CastRays(rays_dev.GetData(), int(n), t_dev.GetData(), status_dev.GetData(), samples_dev.GetData());
  Hits hits;
  hits.t.resize(n);
  hits.status.resize(n);
  hits.samples.resize(n);
  t_dev.CopyToHost(hits.t.data());
  status_dev.CopyToHost(hits.status.data());
  samples_dev.CopyToHost(reinterpret_cast<Voxel*>(hits.samples.data()));
  return hits;
}

// The ranges come from CastRays on a volume fused from a depth image; a second volume is then built from the rays alone.
TEST(ColorRays, AMapFromRaysHasColours)
{
  const Frame frame = BumpsFrame(Transform());
  auto scene = Fused(8192, 2048, frame, 2);
  const std::vector<Ray> rays = PixelRays(frame);
  const int count = int(rays.size());
  Buffer<Ray> rays_dev(rays.size());
  rays_dev.CopyFromHost(rays.data());
  const Hits seen = Cast(*scene, rays_dev);
  std::vector<Vector3f> colors(rays.size());
  int measured = 0;
  for (int i = 0; i < count; ++i)
  {
    colors[i] = Paint(Along(rays[i], seen.t[i]));
    measured += seen.status[i] == VK_RAY_HIT ? 1 : 0;                    // a miss reports t == 0: no measurement
  }
  ASSERT_TRUE(measured * 20 >= count * 19);
  Buffer<float> ranges_dev(rays.size());
  Buffer<Vector3f> colors_dev(rays.size());
  ranges_dev.CopyFromHost(seen.t.data());
  colors_dev.CopyFromHost(colors.data());

  auto volume = Fresh(4093, 2048);
  IntegrateRaysOptions fuse;
  fuse.one_observation = true;
  const IntegrateRaysCounts fused = volume->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), count, nullptr, fuse);
  ASSERT_EQ(measured, fused.integrated);
  ASSERT_EQ(0, fused.lost);
  const int allocated = volume->GetAllocatedBlockCount();

  // the control: a map from rays has no colour until ColorRays gives it one
  Hits hits = Cast(*volume, rays_dev);
  int hit = 0, carries = 0;
  for (int i = 0; i < count; ++i)
  {
    hit += hits.status[i] == VK_RAY_HIT ? 1 : 0;
    carries += hits.samples[i].color_weight != 0 ? 1 : 0;
  }
  ASSERT_TRUE(hit * 20 >= measured * 19);
  ASSERT_EQ(0, carries);

  const std::vector<vk_voxel> was = Voxels(*volume);
  ColorRaysOptions paint;
  paint.one_observation = true;
  const ColorRaysCounts counts = volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), count, nullptr, paint);
  std::printf("         %d rays coloured, %d without a colour, %d without a measurement, %d invalid; %d blocks and %d voxels updated, "
      "%d voxels not near a surface, %u visits lost\n", counts.coloured, counts.colourless, counts.unmeasured, counts.invalid,
      counts.blocks, counts.voxels, counts.not_near, counts.lost);
  ASSERT_EQ(measured, counts.coloured);
  ASSERT_EQ(count - measured, counts.unmeasured);
  ASSERT_EQ(0, counts.colourless + counts.invalid);
  ASSERT_EQ(0u, counts.lost);                                            // IntegrateRays allocated every block of the same band
  ASSERT_TRUE(counts.blocks > 500 && counts.voxels > 50000 && counts.not_near > 0);
  ASSERT_EQ(allocated, volume->GetAllocatedBlockCount());              // the call allocates nothing
  // distances and their weights keep their bytes; as many voxels as counted took a colour weight of 1
  const std::vector<vk_voxel> now = Voxels(*volume);
  int coloured_voxels = 0;
  for (size_t i = 0; i < now.size(); ++i)
  {
    ASSERT_TRUE(std::memcmp(&was[i].distance, &now[i].distance, sizeof(float)) == 0 && was[i].distance_weight == now[i].distance_weight);
    if (now[i].color_weight != 0)
    {
      ASSERT_TRUE(now[i].color_weight == 1 && std::fabs(now[i].distance) < 1.0f);
      ++coloured_voxels;
    }
  }
  ASSERT_EQ(counts.voxels, coloured_voxels);

  // CastRays sees the colours of the rays
  hits = Cast(*volume, rays_dev);
  hit = carries = 0;
  float worst = 0.0f;
  for (int i = 0; i < count; ++i)
  {
    if (hits.status[i] != VK_RAY_HIT) continue;
    ++hit;
    if (hits.samples[i].color_weight == 0) continue;
    ++carries;
    worst = std::max(worst, Difference(hits.samples[i].color, Paint(Along(rays[i], hits.t[i]))));
  }
  std::printf("         %d of %d rays hit, %d samples carry a colour weight, at worst %.4f from the paint at the hit\n", hit, count,
      carries, worst);
  ASSERT_TRUE(carries * 20 >= measured * 19);
  ASSERT_TRUE(worst <= kCastBound);

  // and so does the mesh
  Extractor extractor(volume);
  extractor.SetAllAllocated(true);
  extractor.SetColors(true);
  Mesh mesh;
  extractor.Extract(mesh);
  ASSERT_TRUE(mesh.points.size() > 10000);
  ASSERT_EQ(mesh.points.size(), mesh.colors.size());
  size_t with_colour = 0;
  worst = 0.0f;
  for (size_t i = 0; i < mesh.points.size(); ++i)
  {
    const Vector3f& c = mesh.colors[i];
    if (c[0] == 0.0f && c[1] == 0.0f && c[2] == 0.0f) continue;       // no colour: the paint is nowhere (0, 0, 0)
    ++with_colour;
    const float color[3] = {c[0], c[1], c[2]};
    worst = std::max(worst, Difference(color, Paint(mesh.points[i])));
  }
  std::printf("         %zu of %zu vertices carry a colour, at worst %.4f from the paint at the vertex\n", with_colour,
      mesh.points.size(), worst);
  ASSERT_TRUE(with_colour * 20 >= mesh.points.size() * 19);
  ASSERT_TRUE(worst <= kMeshBound);

  // what the C ABI refuses arrives as an exception
  ASSERT_THROW(volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), nullptr, 8));
  ASSERT_THROW(volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), -1));
  ColorRaysOptions bad;
  bad.band = -1.0f;
  ASSERT_THROW(volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), 8, nullptr, bad));
  bad = ColorRaysOptions();
  bad.band = 65 * kVoxel;
  ASSERT_THROW(volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), 8, nullptr, bad));
  bad = ColorRaysOptions();
  bad.max_color_weight = 0.5f;
  ASSERT_THROW(volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), 8, nullptr, bad));
}

// between SetView calls only: not while Tracer::Trace(keyframe, next_frame) has the next frame's requests in the volume. The
// visible list of the last SetView survives the call.
TEST(ColorRays, RefusedWhileAFrameIsAnnounced)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  const std::vector<Ray> rays = PixelRays(frame);
  std::vector<float> ranges(rays.size());
  std::vector<Vector3f> colors(rays.size(), Vector3f(0.25f, 0.5f, 1.0f));
  for (int y = 0; y < kHeight; ++y)                                       // the depth of a pixel is the z of its point
    for (int x = 0; x < kWidth; ++x) ranges[size_t(y) * kWidth + x] = Bumps(x, y) * Length(rays[size_t(y) * kWidth + x].direction);
  Buffer<Ray> rays_dev(rays.size());
  Buffer<float> ranges_dev(ranges.size());
  Buffer<Vector3f> colors_dev(colors.size());
  rays_dev.CopyFromHost(rays.data());
  ranges_dev.CopyFromHost(ranges.data());
  colors_dev.CopyFromHost(colors.data());
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  const ColorRaysCounts counts = volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), int(rays.size()));
  ASSERT_EQ(int(rays.size()), counts.coloured);
  ASSERT_TRUE(counts.voxels > 10000);
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());

  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = BumpsFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const std::vector<vk_voxel> was = Voxels(*volume);
  ASSERT_THROW(volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), int(rays.size())));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
  volume->CancelRequestsAhead(3);
  const ColorRaysCounts after = volume->ColorRays(rays_dev.GetData(), ranges_dev.GetData(), colors_dev.GetData(), int(rays.size()));
  ASSERT_EQ(int(rays.size()), after.coloured);
}

// no rays: nothing is launched, nothing changes, the visible list stays
TEST(ColorRays, NoRaysAreNoCall)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 1);
  const int before = volume->GetAllocatedBlockCount();
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  const std::vector<vk_voxel> was = Voxels(*volume);
  const ColorRaysCounts counts = volume->ColorRays(nullptr, nullptr, nullptr, 0);
  ASSERT_EQ(0, counts.coloured + counts.colourless + counts.unmeasured + counts.invalid + counts.blocks + counts.voxels + counts.not_near);
  ASSERT_EQ(0u, counts.lost);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
}

int main(int argc, char** argv) { return RunTests("color_rays_tests", argc, argv); }
