// cast_tests.cpp — Volume::CastRays(rays, count, t, status, samples, gradients, pose) through the C++ class layer -> C ABI -> HIP
// kernel (no upstream case: the reference casts only the pixel rays of one pinhole camera). The call is held against the CPU
// statement bit for bit by tests/test_gpu_cast.py; these cases are what a user of the class sees: rays built from the Tracer's
// camera hit where the raycast depth says, a ray from behind a surface reports no back face, and after Merge(other, pose) the
// rays see both sessions' surfaces. Harness: volume_test_support.h.
//
//   ./cast_tests            run everything (needs a GPU)
//   ./cast_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// |t (n . optical axis) - raycast depth| in metres, tests/test_cast_reference.py: twice what the statement measures against
// the reference's raycast. The maximum is reached where the observed region ends (the rim of the image, a block the table
// could not hold): there the reference's trilinear sample blends the unobserved voxels in and the cast's does not
static const float kDepthBound = 2 * 0.0232f;

struct Hits
{
  std::vector<float> t;
  std::vector<int> status;
  std::vector<vk_voxel> samples;
  std::vector<Vector4f> gradients;
  int Count(int outcome) const { return int(std::count(status.begin(), status.end(), outcome)); }
};

static Hits Cast(const Volume& volume, const std::vector<Ray>& rays, const Transform* pose = nullptr, const CastOptions& options = CastOptions())
{
  const size_t n = rays.size();
  Buffer<Ray> rays_dev(n);
  Buffer<float> t_dev(n);
  Buffer<int> status_dev(n);
  Buffer<Voxel> samples_dev(n);
  Buffer<Vector4f> gradients_dev(n);
  rays_dev.CopyFromHost(rays.data());
  volume.CastRays(rays_dev.GetData(), int(n), t_dev.GetData(), status_dev.GetData(), samples_dev.GetData(), gradients_dev.GetData(), pose, options);
  Hits hits;
  hits.t.resize(n);
  hits.status.resize(n);
  hits.samples.resize(n);
  hits.gradients.resize(n);
  t_dev.CopyToHost(hits.t.data());
  status_dev.CopyToHost(hits.status.data());
  samples_dev.CopyToHost(reinterpret_cast<Voxel*>(hits.samples.data()));
  gradients_dev.CopyToHost(hits.gradients.data());
  return hits;
}

// the raycast of the fusing view and the same pixels as rays: where both hit, t along the optical axis is the raycast's depth
TEST(Cast, CameraRaysHitWhereTheRaycastSays)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);
  Frame traced;
  traced.depth_projection = traced.color_projection = frame.depth_projection;
  traced.depth_image = std::make_shared<Image>(kWidth, kHeight);
  Tracer tracer(volume);
  tracer.Trace(traced);
  std::vector<float> depths(traced.depth_image->GetTotal());
  traced.depth_image->CopyToHost(depths.data());

  const std::vector<Ray> rays = PixelRays(frame);
  const Hits hits = Cast(*volume, rays);
  int seen = 0, lost = 0, both = 0, sampled = 0, whole = 0;
  float worst = 0.0f, worst_whole = 0.0f;
  for (int y = 0; y < kHeight; ++y)
    for (int x = 0; x < kWidth; ++x)
    {
      const size_t i = size_t(y) * kWidth + x;
      const bool hit = hits.status[i] == VK_RAY_HIT;
      if (hit)
      {
        ASSERT_TRUE(hits.t[i] > 0.0f);
        // where the hit has a sample it lies on the surface (at the end of the observed region it may have none)
        if (hits.samples[i].distance_weight != 0) { ++sampled; ASSERT_TRUE(std::fabs(hits.samples[i].distance) < 0.05f); }
        else ASSERT_TRUE(hits.samples[i].distance == 1.0f);
      }
      else ASSERT_TRUE(hits.t[i] == 0.0f && hits.samples[i].distance == 1.0f && hits.samples[i].distance_weight == 0);
      if (!(depths[i] > 0.0f)) continue;
      ++seen;
      if (!hit) { ++lost; continue; }
      ++both;
      const float error = std::fabs(hits.t[i] * rays[i].direction[2] / Length(rays[i].direction) - depths[i]);
      worst = std::fmax(worst, error);
      // all eight voxels around the hit observed: both samples read the same eight values
      if (hits.gradients[i][3] == 1.0f) { ++whole; worst_whole = std::fmax(worst_whole, error); }
    }
  std::printf("         raycast depth at %d pixels, %d of them no hit of a ray; both at %d: worst |dz| %g m; hits with a sample %d, "
      "with all eight voxels observed %d: worst |dz| %g m\n", seen, lost, both, worst, sampled, whole, worst_whole);
  ASSERT_TRUE(seen > kWidth * kHeight / 2);
  ASSERT_TRUE(lost * 20 <= seen);
  ASSERT_TRUE(worst <= kDepthBound);
  ASSERT_TRUE(sampled > kWidth * kHeight / 2 && whole > kWidth * kHeight / 2);
  // what the C ABI refuses arrives as an exception
  Buffer<Ray> rays_dev(8);
  Buffer<float> t_dev(8);
  Buffer<int> status_dev(8);
  ASSERT_THROW(volume->CastRays(rays_dev.GetData(), 8, nullptr, status_dev.GetData()));
  ASSERT_THROW(volume->CastRays(rays_dev.GetData(), -1, t_dev.GetData(), status_dev.GetData()));
  CastOptions bad;
  bad.max_steps = 0;
  ASSERT_THROW(volume->CastRays(rays_dev.GetData(), 8, t_dev.GetData(), status_dev.GetData(), nullptr, nullptr, nullptr, bad));
  volume->CastRays(nullptr, 0, t_dev.GetData(), status_dev.GetData());
}

// the twin of every pixel ray that hits: from 3 voxels behind the hit, back at the camera. It starts inside the wall,
// walks out through the surface and must not report it: the surface was not crossed from its observed free side
TEST(Cast, ARayFromBehindReportsNoBackFace)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);
  const std::vector<Ray> rays = PixelRays(frame);
  const Hits hits = Cast(*volume, rays);
  std::vector<Ray> twins;
  for (size_t i = 0; i < rays.size(); ++i)
  {
    if (hits.status[i] != VK_RAY_HIT) continue;
    const float scale = (hits.t[i] + 3 * kVoxel) / Length(rays[i].direction);
    Ray twin;
    twin.origin = Vector3f(scale * rays[i].direction[0], scale * rays[i].direction[1], scale * rays[i].direction[2]);
    twin.direction = Vector3f(-rays[i].direction[0], -rays[i].direction[1], -rays[i].direction[2]);
    twins.push_back(twin);
  }
  ASSERT_TRUE(twins.size() > size_t(kWidth) * kHeight / 2);
  const Hits back = Cast(*volume, twins);
  int reported = 0;
  for (size_t i = 0; i < twins.size(); ++i)
    if (back.status[i] == VK_RAY_HIT && back.t[i] < 4 * kVoxel) ++reported;
  std::printf("         %zu twins: %d miss, %d hit, %d of them at the back face\n", twins.size(), back.Count(VK_RAY_MISS), back.Count(VK_RAY_HIT), reported);
  ASSERT_EQ(0, reported);
  ASSERT_EQ(0, back.Count(VK_RAY_INVALID));
}

// two sessions: the wall seen by one camera, and the same wall seen by a camera 1.3 m to the side, in a volume of its own.
// Before the merge the first map does not know the second wall; after Merge(other, pose) rays given in the second camera's
// frame, carried by the pose, hit it where they hit in the second session's own volume — the resampled field moves its
// zero crossing by a fraction of a voxel (half a voxel bounds the mean, as in merge_pose_tests) — and the first
// session's rays hit what they hit before.
TEST(Cast, AfterAMergeBothSessionsSurfacesAreSeen)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(4093, 4096, frame, 2);
  auto other = Fused(509, 4096, frame, 2);
  const Transform pose = Transform::Translate(1.3f, 0.0f, 0.0f);
  const std::vector<Ray> rays = PixelRays(frame);
  const Hits first_before = Cast(*volume, rays), second_alone = Cast(*other, rays), second_before = Cast(*volume, rays, &pose);
  ASSERT_TRUE(first_before.Count(VK_RAY_HIT) > kWidth * kHeight / 2 && second_alone.Count(VK_RAY_HIT) > kWidth * kHeight / 2);
  ASSERT_EQ(0, second_before.Count(VK_RAY_HIT));

  const MergePoseCounts counts = volume->Merge(*other, pose);
  ASSERT_EQ(0, counts.left_out);
  const Hits first_after = Cast(*volume, rays), second_after = Cast(*volume, rays, &pose);
  int kept = 0, found = 0, wanted = 0;
  double moved = 0;
  for (size_t i = 0; i < rays.size(); ++i)
  {
    ASSERT_EQ(first_before.status[i], first_after.status[i]);
    ASSERT_TRUE(std::fabs(first_before.t[i] - first_after.t[i]) <= 1e-6f);
    if (first_after.status[i] == VK_RAY_HIT) ++kept;
    if (second_alone.status[i] != VK_RAY_HIT) continue;
    ++wanted;
    if (second_after.status[i] != VK_RAY_HIT) continue;
    ++found;
    moved += std::fabs(second_after.t[i] - second_alone.t[i]);
  }
  std::printf("         first session: %d hits kept; second session: %d of %d hits found in the merged map, mean |dt| %.5f m\n",
      kept, found, wanted, found ? moved / found : 0.0);
  ASSERT_TRUE(found * 10 >= wanted * 9);
  ASSERT_TRUE(moved / found < 0.004);
}

int main(int argc, char** argv) { return RunTests("cast_tests", argc, argv); }
