// register_tests.cpp — Volume::Register(other, start) through the C++ class layer -> C ABI -> HIP kernels (no upstream case:
// the reference's Volume is a process-wide singleton, src/volume.cu:17-21). The call's terms, sums and loop are held against
// the CPU statement by tests/test_gpu_register.py; these cases are what a user of the class sees: a copy is registered as
// it stands, a source carried by whole blocks has no residual at that shift, and a source displaced by a generic pose is
// brought back from the identity and then merges as the surface it came from. Harness: volume_test_support.h.
//
//   ./register_tests            run everything (needs a GPU)
//   ./register_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

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

// a volume against itself and against a copy in a table of another size: no residual, no gradient, one step, the pose's bytes kept
TEST(Register, ACloneIsAlreadyRegistered)
{
  auto volume = Fused(509, 4096, BumpsFrame(Transform()), 2);
  const Registration self = volume->Register(*volume, Transform());
  ASSERT_EQ(1, self.steps);
  ASSERT_TRUE(self.converged && self.overlap);
  ASSERT_TRUE(self.residuals > 100000);
  ASSERT_EQ(0.0f, self.rms);
  ASSERT_TRUE(SameMatrices(self.pose, Transform()));
  auto copy = Fresh(4093, 2048);
  copy->Merge(*volume);
  const Registration other = volume->Register(*copy, Transform());
  ASSERT_EQ(1, other.steps);
  ASSERT_TRUE(other.converged && other.overlap);
  ASSERT_EQ(self.residuals, other.residuals);
  ASSERT_EQ(0.0f, other.rms);
  ASSERT_TRUE(SameMatrices(other.pose, Transform()));
  // nowhere near: no voxel to compare, and the pose stays what it was
  const Transform apart = Transform::Translate(10.0f, 0.0f, 0.0f);
  const Registration none = volume->Register(*copy, apart);
  ASSERT_EQ(1, none.steps);
  ASSERT_TRUE(!none.converged && !none.overlap);
  ASSERT_EQ(0, none.residuals);
  ASSERT_TRUE(SameMatrices(none.pose, apart));
  ASSERT_THROW(volume->Register(*copy, Transform(), 0));
  ASSERT_THROW(volume->Register(*copy, Transform(), 20, 1.5f));
}

// the source is the volume carried one block down in x and two up in y: at the pose that carries it back every sample is a voxel
TEST(Register, ABlockShiftHasNoResidual)
{
  auto volume = Fused(509, 4096, BumpsFrame(Transform()), 2);
  const Transform shift = Transform::Translate(8.0f * 0.008f, -16.0f * 0.008f, 0.0f);
  auto source = Fresh(1021, 2048);
  const MergePoseCounts moved = source->Merge(*volume, shift.Inverse());
  ASSERT_EQ(0, moved.left_out);
  const Registration got = volume->Register(*source, shift);
  std::printf("         %d residuals, rms %g, %d step(s)\n", got.residuals, got.rms, got.steps);
  ASSERT_TRUE(got.residuals > 100000);
  ASSERT_EQ(0.0f, got.rms);
  ASSERT_EQ(1, got.steps);
  ASSERT_TRUE(got.converged);
  ASSERT_TRUE(SameMatrices(got.pose, shift));
}

// the source is the volume resampled into a frame displaced by a generic pose; from the identity — 26 mm and 11 degrees off
// — the registration finds the pose well below a voxel (the bounds of tests/test_register_reference.py: a thirty-second of
// a voxel and 0.05 degrees), and the source merged through it raycasts as the surface both were fused from
TEST(Register, AGenericPoseThenTheMerge)
{
  const Frame frame = BumpsFrame(Transform());
  auto volume = Fused(509, 4096, frame, 2);
  const float yaw = 0.5f * 0.17453293f, pitch = 0.5f * 0.08726646f;   // 10 and 5 degrees
  const Transform truth = Transform::Translate(0.013f, -0.021f, 0.008f) * Transform::Rotate(std::cos(yaw), 0.0f, std::sin(yaw), 0.0f) *
      Transform::Rotate(std::cos(pitch), std::sin(pitch), 0.0f, 0.0f);
  auto source = Fresh(4093, 4096);
  ASSERT_EQ(0, source->Merge(*volume, truth.Inverse()).left_out);
  const Registration got = volume->Register(*source, Transform());
  double metres = 0, degrees = 0;
  PoseError(got.pose, truth, &metres, &degrees);
  std::printf("         %d step(s), %d residuals, rms %g; %.3g m and %.3g degrees from the pose\n", got.steps, got.residuals, got.rms, metres, degrees);
  ASSERT_TRUE(got.converged && got.overlap);
  ASSERT_TRUE(got.steps <= 20);
  ASSERT_TRUE(metres < 0.25e-3 && degrees < 0.05);

  auto merged = Fresh(8192, 4096);
  const MergePoseCounts counts = merged->Merge(*source, got.pose);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.sampled > 100000);
  merged->SetView(frame, 3);
  Frame traced;
  traced.depth_to_world_transform = Transform();
  traced.depth_projection = traced.color_projection = frame.depth_projection;
  traced.depth_image = std::make_shared<Image>(kWidth, kHeight);
  Tracer tracer(merged);
  tracer.Trace(traced);
  std::vector<float> depths(traced.depth_image->GetTotal());
  traced.depth_image->CopyToHost(depths.data());
  int hits = 0;
  double error = 0;
  for (int y = 0; y < kHeight; ++y)
    for (int x = 0; x < kWidth; ++x)
    {
      const float depth = depths[size_t(y) * kWidth + x];
      if (!(depth > 0)) continue;
      ++hits;
      error += std::fabs(depth - Bumps(x, y));
    }
  std::printf("         %d of %d pixels hit, mean |depth error| %.5f m\n", hits, kWidth * kHeight, hits ? error / hits : 0.0);
  ASSERT_TRUE(hits > kWidth * kHeight / 2);
  ASSERT_TRUE(error / hits < 0.004);                 // half a voxel, as merge_pose_tests' raycast
}

int main(int argc, char** argv) { return RunTests("register_tests", argc, argv); }
