// register_rays_tests.cpp — Volume::RegisterRays(rays, ranges, count, start, options) through the C++ class layer -> C ABI -> HIP
// kernels (no upstream case: the reference tracks only pinhole depth images against a raycast keyframe). The call is held
// against the CPU statement by tests/test_gpu_register_rays.py; these cases are what a user of the class sees: the rays of a
// camera with the ranges CastRays gives them, handed over in a sensor frame displaced by a generic pose, are registered from
// the identity and fused at the pose found; no rays are no call; and, since the call only reads, a volume with an announced
// frame does not refuse. Harness: volume_test_support.h.
//
//   ./register_rays_tests            run everything (needs a GPU)
//   ./register_rays_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// the bounds of tests/test_register_rays_reference.py for this scene and this pose: the statement ends 0.065 mm and 0.0082
// degrees from the truth, the distance between CastRays' hit and the zero set of the trilinear field
static const double kMetresBound = 0.1e-3, kDegreesBound = 0.012;

static bool SameMatrices(const Transform& a, const Transform& b)
{
  const vk_transform x = a.ToVk(), y = b.ToVk();
  return std::memcmp(&x, &y, sizeof(x)) == 0;
}

// (metres, degrees) between two poses
static void PoseError(const Transform& pose, const Transform& truth, double* metres, double* degrees)
{
  const vk_transform delta = (truth.Inverse() * pose).ToVk(), a = pose.ToVk(), b = truth.ToVk();
  const double sx = 0.5 * (delta.m[6] - delta.m[9]), sy = 0.5 * (delta.m[8] - delta.m[2]), sz = 0.5 * (delta.m[1] - delta.m[4]);
  const double cosine = 0.5 * (double(delta.m[0]) + delta.m[5] + delta.m[10] - 1.0);
  *degrees = std::atan2(std::sqrt(sx * sx + sy * sy + sz * sz), cosine) * 180.0 / 3.14159265358979323846;
  const double dx = double(a.m[12]) - b.m[12], dy = double(a.m[13]) - b.m[13], dz = double(a.m[14]) - b.m[14];
  *metres = std::sqrt(dx * dx + dy * dy + dz * dz);
}

// 26 mm and 11 degrees from the identity
static Transform GenericPose()
{
  const float yaw = 0.5f * 0.17453293f, pitch = 0.5f * 0.08726646f;   // 10 and 5 degrees
  return Transform::Translate(0.013f, -0.021f, 0.008f) * Transform::Rotate(std::cos(yaw), 0.0f, std::sin(yaw), 0.0f) *
      Transform::Rotate(std::cos(pitch), std::sin(pitch), 0.0f, 0.0f);
}

// the rays of the volume's frame as the sensor at `pose` (Tvolume_rays) holds them: through the inverse, in double
static std::vector<Ray> InSensorFrame(const std::vector<Ray>& rays, const Transform& pose)
{
  const vk_transform t = pose.ToVk();
  std::vector<Ray> out(rays.size());
  for (size_t i = 0; i < rays.size(); ++i)
    for (int a = 0; a < 3; ++a)
    {
      double o = t.inv[12 + a], d = 0.0;
      for (int c = 0; c < 3; ++c)
      {
        o += double(t.inv[4 * c + a]) * rays[i].origin[c];
        d += double(t.inv[4 * c + a]) * rays[i].direction[c];
      }
      out[i].origin[a] = float(o);
      out[i].direction[a] = float(d);
    }
  return out;
}

struct Sweep
{
  std::vector<Ray> rays;            // in the volume's frame
  std::vector<float> ranges;        // CastRays' t: 0 without a hit
  int hits;
};

static Sweep CastSweep(const Volume& volume, const Frame& frame, const Transform* pose = nullptr)
{
  Sweep s;
  s.rays = PixelRays(frame);
  const int count = int(s.rays.size());
  Buffer<Ray> rays_dev(s.rays.size());
  Buffer<float> t_dev(s.rays.size());
  Buffer<int> status_dev(s.rays.size());
  rays_dev.CopyFromHost(s.rays.data());
  volume.CastRays(rays_dev.GetData(), count, t_dev.GetData(), status_dev.GetData(), nullptr, nullptr, pose);
  s.ranges.resize(s.rays.size());
  t_dev.CopyToHost(s.ranges.data());
  s.hits = 0;
  for (float t : s.ranges) s.hits += t > 0.0f ? 1 : 0;
  return s;
}

// a camera's rays with CastRays' ranges, seen from a sensor 26 mm and 11 degrees away, are registered from the identity; the
// sweep is then fused at the pose found and CastRays, from the true pose, finds the surface where the map has it
TEST(RegisterRays, ADisplacedSweepIsLocalisedThenFused)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);
  const Sweep sweep = CastSweep(*volume, frame);
  const int count = int(sweep.rays.size());
  ASSERT_TRUE(sweep.hits > count * 9 / 10);
  const Transform truth = GenericPose();
  const std::vector<Ray> seen = InSensorFrame(sweep.rays, truth);
  Buffer<Ray> rays_dev(seen.size());
  Buffer<float> ranges_dev(sweep.ranges.size());
  rays_dev.CopyFromHost(seen.data());
  ranges_dev.CopyFromHost(sweep.ranges.data());

  const std::vector<vk_voxel> was = Voxels(*volume);
  const Volume& map = *volume;                       // the call is const on the volume
  const Registration got = map.RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), count, Transform());
  double metres = 0, degrees = 0;
  PoseError(got.pose, truth, &metres, &degrees);
  std::printf("         %d step(s), %d residuals of %d returns, rms %g; %.3g m and %.3g degrees from the pose\n", got.steps, got.residuals,
      sweep.hits, got.rms, metres, degrees);
  ASSERT_TRUE(got.converged && got.overlap);
  ASSERT_TRUE(got.steps <= 10);
  ASSERT_TRUE(got.residuals > sweep.hits * 9 / 10);
  ASSERT_TRUE(metres < kMetresBound && degrees < kDegreesBound);
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);

  // localise, then map: the sweep fused at the pose found
  auto second = Fresh(4093, 4096);
  IntegrateRaysOptions fuse;
  const IntegrateRaysCounts fused = second->IntegrateRays(rays_dev.GetData(), ranges_dev.GetData(), count, &got.pose, fuse);
  ASSERT_EQ(sweep.hits, fused.integrated);
  Buffer<float> t_dev(seen.size());
  Buffer<int> status_dev(seen.size());
  second->CastRays(rays_dev.GetData(), count, t_dev.GetData(), status_dev.GetData(), nullptr, nullptr, &truth);
  std::vector<float> again(seen.size());
  t_dev.CopyToHost(again.data());
  int both = 0;
  float worst = 0.0f;
  for (size_t i = 0; i < again.size(); ++i)
  {
    if (!(again[i] > 0.0f) || !(sweep.ranges[i] > 0.0f)) continue;
    ++both;
    worst = std::fmax(worst, std::fabs(again[i] - sweep.ranges[i]));
  }
  std::printf("         %d returns, %d of them hit in the second volume: worst |dt| %g m\n", sweep.hits, both, worst);
  ASSERT_TRUE(both * 20 >= sweep.hits * 19);
  ASSERT_TRUE(worst <= kVoxel);

  // ten metres away nothing is compared and the pose stays what it was
  const Transform apart = Transform::Translate(10.0f, 0.0f, 0.0f) * truth;
  const Registration none = map.RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), count, apart);
  ASSERT_EQ(1, none.steps);
  ASSERT_TRUE(!none.converged && !none.overlap);
  ASSERT_EQ(0, none.residuals);
  ASSERT_TRUE(SameMatrices(none.pose, apart));
  // what the C ABI refuses arrives as an exception
  ASSERT_THROW(map.RegisterRays(rays_dev.GetData(), nullptr, 8, Transform()));
  ASSERT_THROW(map.RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), -1, Transform()));
  RegisterRaysOptions bad;
  bad.iterations = 65;
  ASSERT_THROW(map.RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), 8, Transform(), bad));
  bad = RegisterRaysOptions();
  bad.max_abs_distance = 1.5f;
  ASSERT_THROW(map.RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), 8, Transform(), bad));
}

// no rays: nothing is launched, nothing changes, the start comes back
TEST(RegisterRays, NoRaysAreNoCall)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 1);
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  const std::vector<vk_voxel> was = Voxels(*volume);
  const Transform start = GenericPose();
  const Registration none = volume->RegisterRays(nullptr, nullptr, 0, start);
  ASSERT_EQ(0, none.steps);
  ASSERT_EQ(0, none.residuals);
  ASSERT_TRUE(!none.converged && !none.overlap);
  ASSERT_TRUE(SameMatrices(none.pose, start));
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
}

// the call writes nothing of the volume: like Sample and CastRays it runs while Tracer::Trace(keyframe, next_frame) has the next
// frame's requests in the volume, gives what it gave before, and leaves the announcement standing
TEST(RegisterRays, AllowedWhileAFrameIsAnnounced)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 2);
  const Sweep sweep = CastSweep(*volume, frame);
  const int count = int(sweep.rays.size());
  const Transform truth = GenericPose();
  const std::vector<Ray> seen = InSensorFrame(sweep.rays, truth);
  Buffer<Ray> rays_dev(seen.size());
  Buffer<float> ranges_dev(sweep.ranges.size());
  rays_dev.CopyFromHost(seen.data());
  ranges_dev.CopyFromHost(sweep.ranges.data());
  const Registration before = volume->RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), count, Transform());
  ASSERT_TRUE(before.converged);

  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = BumpsFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const int blocks = volume->GetAllocatedBlockCount();
  const Registration during = volume->RegisterRays(rays_dev.GetData(), ranges_dev.GetData(), count, Transform());
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(blocks, volume->GetAllocatedBlockCount());
  ASSERT_EQ(before.steps, during.steps);
  ASSERT_EQ(before.residuals, during.residuals);
  ASSERT_TRUE(during.converged && SameMatrices(before.pose, during.pose));
  volume->CancelRequestsAhead(3);
}

int main(int argc, char** argv) { return RunTests("register_rays_tests", argc, argv); }
