// integrate_rays_tests.cpp — Volume::IntegrateRays(rays, ranges, count, pose, options) through the C++ class layer -> C ABI -> HIP
// kernels (no upstream case: the reference fuses only the pixels of one pinhole depth image). The call is held against the CPU
// statement bit for bit by tests/test_gpu_integrate_rays.py; these cases are what a user of the class sees: the rays of the
// Tracer's camera with the ranges of its depth image, fused into a second Volume, raycast there where they were measured; a
// volume with an announced frame refuses; no rays are no call. Harness: volume_test_support.h.
//
//   ./integrate_rays_tests            run everything (needs a GPU)
//   ./integrate_rays_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// |raycast depth of the rays' volume - the depth the rays carried| in metres, tests/test_integrate_rays_reference.py: twice what
// the statement measures between the reference's integrator and the rays of the same depth frame. The maximum is reached on the
// rim of the image, where the observed region ends
static const float kDepthBound = 2 * 0.0224f;

static std::vector<float> Raycast(const std::shared_ptr<Volume>& volume, const Frame& frame)
{
  Frame traced;
  traced.depth_projection = traced.color_projection = frame.depth_projection;
  traced.depth_image = std::make_shared<Image>(kWidth, kHeight);
  Tracer tracer(volume);
  tracer.Trace(traced);
  std::vector<float> depths(traced.depth_image->GetTotal());
  traced.depth_image->CopyToHost(depths.data());
  return depths;
}

// the raycast of a fused volume gives a depth image; the camera's pixel rays with range = depth |K^-1 (u, v, 1)| are fused
// into a second, fresh volume, whose raycast at the same view gives the depths back
TEST(IntegrateRays, CameraRaysRebuildTheSurfaceInASecondVolume)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);
  const std::vector<float> depths = Raycast(volume, frame);
  const std::vector<Ray> rays = PixelRays(frame);
  std::vector<float> ranges(rays.size());
  int measured = 0;
  for (size_t i = 0; i < rays.size(); ++i)
  {
    ranges[i] = depths[i] > 0.0f ? depths[i] * Length(rays[i].direction) : 0.0f;       // 0: no measurement
    if (depths[i] > 0.0f) ++measured;
  }
  ASSERT_TRUE(measured > kWidth * kHeight / 2);

  auto second = std::make_shared<Volume>(4093, 4096);
  second->SetVoxelLength(kVoxel);
  Buffer<Ray> rays_dev(rays.size());
  Buffer<float> ranges_dev(ranges.size());
  rays_dev.CopyFromHost(rays.data());
  ranges_dev.CopyFromHost(ranges.data());
  IntegrateRaysOptions options;
  options.one_observation = true;
  const IntegrateRaysCounts counts = second->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size()), nullptr, options);
  std::printf("         %d rays integrated, %d without a measurement, %d invalid; %d blocks allocated in %d rounds, %d blocks and %d voxels "
      "updated, %d visits lost\n", counts.integrated, counts.unmeasured, counts.invalid, counts.allocated, counts.rounds, counts.blocks,
      counts.voxels, counts.lost);
  ASSERT_EQ(measured, counts.integrated);
  ASSERT_EQ(int(rays.size()) - measured, counts.unmeasured);
  ASSERT_EQ(0, counts.invalid);
  ASSERT_EQ(0, counts.lost);
  ASSERT_TRUE(counts.allocated > 100 && counts.blocks > 100 && counts.voxels > 10000 && counts.rounds >= 1);
  ASSERT_EQ(counts.allocated, second->GetAllocatedBlockCount());
  ASSERT_EQ(size_t(0), second->GetVisibleBlocks().GetSize());          // until the next SetView

  // the raycast reads the visible list: the frame the depths make, at the same pose
  Frame seen = frame;
  seen.depth_image = std::make_shared<Image>(kWidth, kHeight);
  seen.depth_image->CopyFromHost(depths.data());
  second->SetView(seen);
  const std::vector<float> again = Raycast(second, frame);
  int both = 0;
  float worst = 0.0f;
  for (size_t i = 0; i < depths.size(); ++i)
  {
    if (!(depths[i] > 0.0f) || !(again[i] > 0.0f)) continue;
    ++both;
    worst = std::fmax(worst, std::fabs(again[i] - depths[i]));
  }
  std::printf("         %d pixels measured, %d of them raycast in the second volume: worst |dz| %g m\n", measured, both, worst);
  ASSERT_TRUE(both * 20 >= measured * 19);
  ASSERT_TRUE(worst <= kDepthBound);

  // a second sweep of the same rays goes on with the running average: the same blocks, nothing allocated
  IntegrateRaysOptions more;
  const IntegrateRaysCounts sweep = second->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size()), nullptr, more);
  ASSERT_EQ(counts.blocks, sweep.blocks);
  ASSERT_EQ(counts.voxels, sweep.voxels);
  ASSERT_EQ(0, sweep.rounds);
  // what the C ABI refuses arrives as an exception
  ASSERT_THROW(second->IntegrateRays(rays_dev.GetData(), nullptr, 8));
  ASSERT_THROW(second->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), -1));
  IntegrateRaysOptions bad;
  bad.max_rounds = 65;
  ASSERT_THROW(second->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), 8, nullptr, bad));
}

// between SetView calls only: not while Tracer::Trace(keyframe, next_frame) has the next frame's requests in the volume
TEST(IntegrateRays, RefusedWhileAFrameIsAnnounced)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = BumpsFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const std::vector<Ray> rays = PixelRays(frame);
  std::vector<float> ranges(rays.size(), 1.0f);
  Buffer<Ray> rays_dev(rays.size());
  Buffer<float> ranges_dev(ranges.size());
  rays_dev.CopyFromHost(rays.data());
  ranges_dev.CopyFromHost(ranges.data());
  const int before = volume->GetAllocatedBlockCount();
  ASSERT_THROW(volume->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size())));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  volume->CancelRequestsAhead(3);
  const IntegrateRaysCounts counts = volume->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), int(rays.size()));
  ASSERT_EQ(int(rays.size()), counts.integrated);
}

// no rays: nothing is launched, nothing changes, the visible list stays
TEST(IntegrateRays, NoRaysAreNoCall)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 1);
  const int before = volume->GetAllocatedBlockCount();
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  std::vector<vk_voxel> was(volume->GetVoxels().GetSize()), now(was.size());
  volume->GetVoxels().CopyToHost(reinterpret_cast<Voxel*>(was.data()));
  const IntegrateRaysCounts counts = volume->IntegrateRays(nullptr, nullptr, 0);
  ASSERT_EQ(0, counts.integrated + counts.unmeasured + counts.invalid + counts.allocated + counts.rounds + counts.blocks + counts.voxels + counts.lost);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());
  volume->GetVoxels().CopyToHost(reinterpret_cast<Voxel*>(now.data()));
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
}

int main(int argc, char** argv) { return RunTests("integrate_rays_tests", argc, argv); }
