// carve_tests.cpp — Volume::CarveRays(rays, ranges, count, pose, options) through the C++ class layer -> C ABI -> HIP kernels (no
// upstream case: the reference writes "free" only into the visible blocks in front of one pinhole depth image). The call is held
// against the CPU statement bit for bit by tests/test_gpu_carve_rays.py; these cases are what a user of the class sees: a wall
// fused from range rays, then measured through — after three sweeps that carve, CastRays sees the wall behind it; a volume
// with an announced frame refuses; no rays are no call. Harness: volume_test_support.h.
//
//   ./carve_tests            run everything (needs a GPU)
//   ./carve_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// |CastRays' t - the range of the back wall| in metres, tests/test_carve_rays_reference.py: twice the maximum the statement
// measures in this scenario
static const float kRangeBound = 2 * 0.00514f;
static const float kFront = 1.0f, kBack = 1.4f;       // two fronto-parallel planes, ten truncation lengths apart

struct Sweep
{
  std::vector<Ray> rays;
  std::vector<float> front, back;
  std::unique_ptr<Buffer<Ray>> rays_dev;
  std::unique_ptr<Buffer<float>> front_dev, back_dev;
};

static Sweep MakeSweep()
{
  Sweep s;
  s.rays = PixelRays(BumpsFrame(Transform()));
  for (const Ray& ray : s.rays)
  {
    s.front.push_back(kFront * Length(ray.direction));
    s.back.push_back(kBack * Length(ray.direction));
  }
  s.rays_dev.reset(new Buffer<Ray>(s.rays.size()));
  s.front_dev.reset(new Buffer<float>(s.rays.size()));
  s.back_dev.reset(new Buffer<float>(s.rays.size()));
  s.rays_dev->CopyFromHost(s.rays.data());
  s.front_dev->CopyFromHost(s.front.data());
  s.back_dev->CopyFromHost(s.back.data());
  return s;
}

// how many rays CastRays reports a hit for, and how many of those nearer than the midpoint of the two walls, within
// kRangeBound of the back wall
static void Cast(const std::shared_ptr<Volume>& volume, const Sweep& s, int& hits, int& near, int& at_back)
{
  const int count = int(s.rays.size());
  Buffer<float> t_dev(count);
  Buffer<int> status_dev(count);
  CastOptions options;
  options.distance_only = true;
  volume->CastRays(s.rays_dev->GetData(), count, t_dev.GetData(), status_dev.GetData(), nullptr, nullptr, nullptr, options);
  std::vector<float> t(count);
  std::vector<int> status(count);
  t_dev.CopyToHost(t.data());
  status_dev.CopyToHost(status.data());
  hits = near = at_back = 0;
  for (int i = 0; i < count; ++i)
  {
    if (status[i] != VK_RAY_HIT) continue;
    ++hits;
    if (t[i] < 0.5f * (s.front[i] + s.back[i])) ++near;
    if (std::fabs(t[i] - s.back[i]) <= kRangeBound) ++at_back;
  }
}

// the front wall is fused once, then the back wall is measured through it three times
static std::shared_ptr<Volume> Scenario(const Sweep& s, bool carving, CarveRaysCounts* last)
{
  auto volume = Fresh(4093, 2048);
  const int count = int(s.rays.size());
  IntegrateRaysOptions fuse;
  fuse.one_observation = true;
  CarveRaysOptions carve;
  carve.one_observation = true;
  const IntegrateRaysCounts first = volume->IntegrateRays(s.rays_dev->GetData(), s.front_dev->GetData(), count, nullptr, fuse);
  ASSERT_EQ(count, first.integrated);
  ASSERT_EQ(0, first.lost);
  for (int sweep = 0; sweep < 3; ++sweep)
  {
    const IntegrateRaysCounts fused = volume->IntegrateRays(s.rays_dev->GetData(), s.back_dev->GetData(), count, nullptr, fuse);
    ASSERT_EQ(count, fused.integrated);
    ASSERT_EQ(0, fused.lost);
    if (carving) *last = volume->CarveRays(s.rays_dev->GetData(), s.back_dev->GetData(), count, nullptr, carve);
  }
  return volume;
}

TEST(CarveRays, AWallThatIsNoLongerThere)
{
  const Sweep s = MakeSweep();
  const int count = int(s.rays.size());
  CarveRaysCounts counts = {};
  auto volume = Scenario(s, true, &counts);
  std::printf("         %d rays carved, %d with nothing to carve, %d without a measurement, %d invalid, %d cut short; %d blocks and %d "
      "voxels updated by %u carves\n", counts.carved, counts.nothing, counts.unmeasured, counts.invalid, counts.cut_short, counts.blocks,
      counts.voxels, counts.carves);
  ASSERT_EQ(count, counts.carved);
  ASSERT_EQ(0, counts.nothing + counts.unmeasured + counts.invalid + counts.cut_short);
  ASSERT_TRUE(counts.blocks > 500 && counts.voxels > 100000 && counts.carves >= unsigned(counts.voxels));
  const int allocated = volume->GetAllocatedBlockCount();
  int hits, near, at_back;
  Cast(volume, s, hits, near, at_back);
  std::printf("         carved: %d of %d rays hit, %d within %g m of the back wall\n", hits, count, at_back, kRangeBound);
  ASSERT_TRUE(at_back * 20 >= count * 19);
  ASSERT_EQ(allocated, volume->GetAllocatedBlockCount());              // a carve allocates nothing

  // the control: without the carves the front wall is still what a ray hits first
  auto stale = Scenario(s, false, &counts);
  Cast(stale, s, hits, near, at_back);
  std::printf("         not carved: %d of %d rays hit, %d nearer than the midpoint of the walls\n", hits, count, near);
  ASSERT_TRUE(near * 20 >= count * 19);
  ASSERT_EQ(allocated, stale->GetAllocatedBlockCount());

  // what the C ABI refuses arrives as an exception
  ASSERT_THROW(volume->CarveRays(s.rays_dev->GetData(), nullptr, 8));
  ASSERT_THROW(volume->CarveRays(s.rays_dev->GetData(), s.back_dev->GetData(), -1));
  CarveRaysOptions bad;
  bad.max_blocks = 4097;
  ASSERT_THROW(volume->CarveRays(s.rays_dev->GetData(), s.back_dev->GetData(), 8, nullptr, bad));
  bad = CarveRaysOptions();
  bad.t_from = -1.0f;
  ASSERT_THROW(volume->CarveRays(s.rays_dev->GetData(), s.back_dev->GetData(), 8, nullptr, bad));
}

// between SetView calls only: not while Tracer::Trace(keyframe, next_frame) has the next frame's requests in the volume. The
// visible list of the last SetView survives a carve.
TEST(CarveRays, RefusedWhileAFrameIsAnnounced)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  const std::vector<Ray> rays = PixelRays(frame);
  std::vector<float> ranges(rays.size(), 2.0f);                          // behind the bumps: the rays pass through them
  Buffer<Ray> rays_dev(rays.size());
  Buffer<float> ranges_dev(ranges.size());
  rays_dev.CopyFromHost(rays.data());
  ranges_dev.CopyFromHost(ranges.data());
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  const CarveRaysCounts counts = volume->CarveRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size()));
  ASSERT_EQ(int(rays.size()), counts.carved);
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
  ASSERT_THROW(volume->CarveRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size())));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
  volume->CancelRequestsAhead(3);
  const CarveRaysCounts after = volume->CarveRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size()));
  ASSERT_EQ(int(rays.size()), after.carved);
}

// no rays: nothing is launched, nothing changes, the visible list stays
TEST(CarveRays, NoRaysAreNoCall)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 1);
  const int before = volume->GetAllocatedBlockCount();
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  const std::vector<vk_voxel> was = Voxels(*volume);
  const CarveRaysCounts counts = volume->CarveRays(nullptr, nullptr, 0);
  ASSERT_EQ(0, counts.carved + counts.nothing + counts.unmeasured + counts.invalid + counts.cut_short + counts.blocks + counts.voxels);
  ASSERT_EQ(0u, counts.carves);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
}

int main(int argc, char** argv) { return RunTests("carve_tests", argc, argv); }
