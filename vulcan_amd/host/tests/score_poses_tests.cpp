// score_poses_tests.cpp — Volume::ScorePoses and Volume::LocalizeRays through the C++ class layer -> C ABI -> HIP kernels (no
// upstream case: the reference tracks only pinhole depth images against a raycast keyframe). The calls are held against the
// CPU statement by tests/test_gpu_score_poses.py; these cases are what a user of the class sees: the rays of a camera with the
// ranges CastRays gives them, handed over in a sensor frame displaced too far for RegisterRays, are localised over a grid of
// candidate poses and fused at the pose found; no rays are no call; and, since the calls only read, a volume with an
// announced frame does not refuse. Harness: volume_test_support.h.
//
//   ./score_poses_tests            run everything (needs a GPU)
//   ./score_poses_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// RegisterRays' bounds (register_rays_tests.cpp, tests/test_register_rays_reference.py): the refinement is its loop, and
// where it ends does not depend on the candidate it started from
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

// translate * yaw * pitch, degrees
static Transform Pose(float x, float y, float z, float yaw_degrees, float pitch_degrees)
{
  const float yaw = 0.5f * yaw_degrees * 0.017453293f, pitch = 0.5f * pitch_degrees * 0.017453293f;
  return Transform::Translate(x, y, z) * Transform::Rotate(std::cos(yaw), 0.0f, std::sin(yaw), 0.0f) *
      Transform::Rotate(std::cos(pitch), std::sin(pitch), 0.0f, 0.0f);
}

// 162 mm and 26 degrees from the identity: too far for RegisterRays
static Transform FarPose() { return Pose(0.12f, -0.09f, 0.06f, 25.0f, -8.0f); }

// 7 yaws x 3 pitches x 5^3 translations: 2 625 candidates, none nearer the truth than 45 mm and 5 degrees
static std::vector<Transform> Grid()
{
  std::vector<Transform> out;
  const float shifts[5] = {-0.16f, -0.08f, 0.0f, 0.08f, 0.16f};
  for (int yaw = -30; yaw <= 30; yaw += 10)
    for (int pitch = -10; pitch <= 10; pitch += 10)
      for (float x : shifts)
        for (float y : shifts)
          for (float z : shifts) out.push_back(Pose(x, y, z, float(yaw), float(pitch)));
  return out;
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

// every `every`th pixel ray of the frame with CastRays' range, in the frame of a sensor at `truth`
struct Sweep
{
  Buffer<Ray> rays_dev;
  Buffer<float> ranges_dev;
  std::vector<float> ranges;
  int count, hits;
};

static void CastSweep(const Volume& volume, const Frame& frame, const Transform& truth, int every, Sweep* s)
{
  const std::vector<Ray> all = PixelRays(frame);
  std::vector<Ray> rays;
  for (size_t i = 0; i < all.size(); i += every) rays.push_back(all[i]);
  s->count = int(rays.size());
  Buffer<Ray> cast_dev(rays.size());
  Buffer<float> t_dev(rays.size());
  Buffer<int> status_dev(rays.size());
  cast_dev.CopyFromHost(rays.data());
  volume.CastRays(cast_dev.GetData(), s->count, t_dev.GetData(), status_dev.GetData(), nullptr, nullptr, nullptr);
  s->ranges.resize(rays.size());
  t_dev.CopyToHost(s->ranges.data());
  s->hits = 0;
  for (float t : s->ranges) s->hits += t > 0.0f ? 1 : 0;
  const std::vector<Ray> seen = InSensorFrame(rays, truth);
  s->rays_dev.Resize(seen.size());
  s->ranges_dev.Resize(seen.size());
  s->rays_dev.CopyFromHost(seen.data());
  s->ranges_dev.CopyFromHost(s->ranges.data());
}

// a sweep seen from a sensor 162 mm and 26 degrees away: RegisterRays from the identity does not find it, LocalizeRays over the
// grid does; the sweep is then fused at the pose found and CastRays, from the true pose, finds the surface where the map has it
TEST(ScorePoses, ASweepFromFarAwayIsLocalisedThenFused)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);
  const Transform truth = FarPose();
  Sweep sweep;
  CastSweep(*volume, frame, truth, 16, &sweep);
  const int count = sweep.count;
  ASSERT_TRUE(sweep.hits > count * 9 / 10);
  const std::vector<Transform> grid = Grid();
  ASSERT_EQ(size_t(2625), grid.size());
  const std::vector<vk_voxel> was = Voxels(*volume);
  const Volume& map = *volume;                       // the calls are const on the volume
  double metres = 0, degrees = 0;

  const Registration alone = map.RegisterRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, Transform());
  PoseError(alone.pose, truth, &metres, &degrees);
  std::printf("         RegisterRays alone: %d step(s), converged %d, overlap %d; %.3g m and %.3g degrees from the pose\n", alone.steps,
      int(alone.converged), int(alone.overlap), metres, degrees);
  ASSERT_TRUE(!(metres < kMetresBound && degrees < kDegreesBound));

  const std::vector<PoseScore> scores = map.ScorePoses(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid);
  ASSERT_EQ(grid.size(), scores.size());
  int best = 0;
  for (size_t k = 0; k < scores.size(); ++k)
  {
    ASSERT_EQ(sweep.hits, scores[k].measured);
    ASSERT_EQ(0, scores[k].invalid);
    ASSERT_TRUE(scores[k].residuals <= scores[k].sampled && scores[k].sampled <= scores[k].measured);
    ASSERT_TRUE(scores[k].sum_squares <= scores[k].sum_abs && scores[k].sum_abs <= (long long)scores[k].residuals << 20);
    const PoseScore& b = scores[size_t(best)];
    if (scores[k].residuals > b.residuals || (scores[k].residuals == b.residuals && scores[k].sum_abs < b.sum_abs)) best = int(k);
  }
  std::printf("         best candidate %d: %d residuals of %d returns, mean |D| %.3g, rms %.3g\n", best, scores[size_t(best)].residuals,
      sweep.hits, scores[size_t(best)].MeanAbs(), scores[size_t(best)].Rms());

  const Localization got = map.LocalizeRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid, sweep.hits / 2);
  PoseError(got.pose, truth, &metres, &degrees);
  std::printf("         LocalizeRays: candidate %d, %d step(s), %d residuals, rms %g; %.3g m and %.3g degrees from the pose\n",
      got.best_index, got.steps, got.residuals, got.rms, metres, degrees);
  ASSERT_EQ(best, got.best_index);
  ASSERT_TRUE(got.converged && got.overlap);
  // the refinement compares more returns than the candidate it started from did, which had at least min_residuals
  ASSERT_TRUE(got.residuals > scores[size_t(best)].residuals && scores[size_t(best)].residuals >= sweep.hits / 2);
  ASSERT_TRUE(metres < kMetresBound && degrees < kDegreesBound);
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);

  // localise, then map: the sweep fused at the pose found hits again within a voxel
  auto second = Fresh(4093, 4096);
  IntegrateRaysOptions fuse;
  const IntegrateRaysCounts fused = second->IntegrateRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, &got.pose, fuse);
  ASSERT_EQ(sweep.hits, fused.integrated);
  Buffer<float> t_dev(sweep.ranges.size());
  Buffer<int> status_dev(sweep.ranges.size());
  second->CastRays(sweep.rays_dev.GetData(), count, t_dev.GetData(), status_dev.GetData(), nullptr, nullptr, &truth);
  std::vector<float> again(sweep.ranges.size());
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

  // no candidate reaches more residuals than there are returns: nothing is chosen and nothing refined
  const Localization none = map.LocalizeRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid, sweep.hits + 1);
  ASSERT_EQ(-1, none.best_index);
  ASSERT_EQ(0, none.steps);
  ASSERT_TRUE(!none.converged && SameMatrices(none.pose, Transform()));
  // what the C ABI refuses arrives as an exception
  ASSERT_THROW(map.ScorePoses(sweep.rays_dev.GetData(), nullptr, 8, grid));
  ASSERT_THROW(map.ScorePoses(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), -1, grid));
  ASSERT_THROW(map.ScorePoses(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), 8, std::vector<Transform>()));
  ASSERT_THROW(map.LocalizeRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), 8, grid, 0));
  ScorePosesOptions bad;
  bad.max_abs_distance = 1.5f;
  ASSERT_THROW(map.ScorePoses(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), 8, grid, bad));
}

// no rays: nothing is launched, nothing changes, every score is empty and nothing is chosen
TEST(ScorePoses, NoRaysAreNoCall)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 1);
  const size_t visible = volume->GetVisibleBlocks().GetSize();
  ASSERT_TRUE(visible > 0);
  const std::vector<vk_voxel> was = Voxels(*volume);
  const std::vector<Transform> poses(3, FarPose());
  const std::vector<PoseScore> scores = volume->ScorePoses(nullptr, nullptr, 0, poses);
  ASSERT_EQ(size_t(3), scores.size());
  for (const PoseScore& s : scores)
  {
    ASSERT_EQ(0, s.measured + s.sampled + s.residuals + s.invalid);
    ASSERT_TRUE(s.sum_abs == 0 && s.sum_squares == 0);
  }
  const Localization none = volume->LocalizeRays(nullptr, nullptr, 0, poses, 1);
  ASSERT_EQ(-1, none.best_index);
  ASSERT_EQ(0, none.steps);
  ASSERT_TRUE(SameMatrices(none.pose, Transform()));
  ASSERT_EQ(visible, volume->GetVisibleBlocks().GetSize());
  const std::vector<vk_voxel> now = Voxels(*volume);
  ASSERT_TRUE(std::memcmp(was.data(), now.data(), was.size() * sizeof(vk_voxel)) == 0);
}

// the calls write nothing of the volume: like Sample and RegisterRays they run while Tracer::Trace(keyframe, next_frame) has the
// next frame's requests in the volume, give what they gave before, and leave the announcement standing
TEST(ScorePoses, AllowedWhileAFrameIsAnnounced)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 2);
  const Transform truth = FarPose();
  Sweep sweep;
  CastSweep(*volume, frame, truth, 16, &sweep);
  const int count = sweep.count;
  const std::vector<Transform> grid = Grid();
  const std::vector<PoseScore> before = volume->ScorePoses(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid);
  const Localization found = volume->LocalizeRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid, sweep.hits / 2);
  ASSERT_TRUE(found.best_index >= 0 && found.converged);

  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = BumpsFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const int blocks = volume->GetAllocatedBlockCount();
  const std::vector<PoseScore> during = volume->ScorePoses(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid);
  const Localization again = volume->LocalizeRays(sweep.rays_dev.GetData(), sweep.ranges_dev.GetData(), count, grid, sweep.hits / 2);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(blocks, volume->GetAllocatedBlockCount());
  ASSERT_EQ(before.size(), during.size());
  for (size_t k = 0; k < before.size(); ++k)
  {
    ASSERT_EQ(before[k].residuals, during[k].residuals);
    ASSERT_TRUE(before[k].sum_abs == during[k].sum_abs && before[k].sum_squares == during[k].sum_squares);
  }
  ASSERT_EQ(found.best_index, again.best_index);
  ASSERT_EQ(found.steps, again.steps);
  ASSERT_TRUE(again.converged && SameMatrices(found.pose, again.pose));
  volume->CancelRequestsAhead(3);
}

int main(int argc, char** argv) { return RunTests("score_poses_tests", argc, argv); }
