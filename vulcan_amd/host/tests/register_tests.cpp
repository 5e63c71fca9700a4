// register_tests.cpp — Volume::Register(other, start) through the C++ class layer -> C ABI -> HIP kernels (no upstream case:
// the reference's Volume is a process-wide singleton, src/volume.cu:17-21). The call's terms, sums and loop are held against
// the CPU statement by tests/test_gpu_register.py; these cases are what a user of the class sees: a copy is registered as
// it stands, a source carried by whole blocks has no residual at that shift, and a source displaced by a generic pose is
// brought back from the identity and then merges as the surface it came from. Harness as in merge_pose_tests.cpp.
//
//   ./register_tests            run everything (needs a GPU)
//   ./register_tests <filter>   run the cases whose name contains <filter>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <array>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <vulcan/vulcan.h>

using namespace vulcan;

struct Failure { std::string text; };

#define STR2(x) #x
#define STR(x) STR2(x)
#define FAIL_HERE(msg) throw Failure{std::string(__FILE__ ":" STR(__LINE__) ": ") + (msg)}
#define ASSERT_TRUE(c) do { if (!(c)) FAIL_HERE("expected true: " #c); } while (0)
#define ASSERT_EQ(a, b) do { if (!((a) == (b))) FAIL_HERE("expected equal: " #a " vs " #b + \
    (" (" + std::to_string((double)(a)) + " vs " + std::to_string((double)(b)) + ")")); } while (0)
#define ASSERT_THROW(stmt) do { bool t__ = false; try { stmt; } catch (const Exception&) { t__ = true; } \
    if (!t__) FAIL_HERE("expected vulcan::Exception: " #stmt); } while (0)

struct TestCase { const char* name; std::function<void()> body; };
static std::vector<TestCase>& Registry() { static std::vector<TestCase> r; return r; }
struct Registrar { Registrar(const char* n, std::function<void()> f) { Registry().push_back({n, f}); } };
#define TEST(suite, name) static void suite##_##name(); \
    static Registrar reg_##suite##_##name(#suite "." #name, suite##_##name); static void suite##_##name()

static const int kWidth = 160, kHeight = 120;

static std::shared_ptr<Image> MakeDepth(const std::function<float(int, int)>& f)
{
  std::vector<float> host(size_t(kWidth) * kHeight);
  for (int y = 0; y < kHeight; ++y) for (int x = 0; x < kWidth; ++x) host[size_t(y) * kWidth + x] = f(x, y);
  auto image = std::make_shared<Image>(kWidth, kHeight);
  image->CopyFromHost(host.data());
  return image;
}

// the scene of tests/register_reference.py: a wall at 1 m with a bump, a dent and a slope — nothing repeats and no direction
// is free, so the alignment has one answer
static float Bumps(int x, int y)
{
  const double w = kWidth, h = kHeight;
  const double bump = std::exp(-((x - 0.375 * w) * (x - 0.375 * w) + (y - 0.42 * h) * (y - 0.42 * h)) / (2 * (0.16 * w) * (0.16 * w)));
  const double dent = std::exp(-((x - 0.69 * w) * (x - 0.69 * w) + (y - 0.67 * h) * (y - 0.67 * h)) / (2 * (0.11 * w) * (0.11 * w)));
  return float(1.0 + 0.06 * bump - 0.04 * dent + 0.03 * x / w);
}

static Frame BumpsFrame(const Transform& pose)
{
  Frame frame;
  frame.depth_projection.SetFocalLength(136, 136);
  frame.depth_projection.SetCenterPoint(80, 60);
  frame.depth_image = MakeDepth(Bumps);
  frame.depth_to_world_transform = pose;
  return frame;
}

static std::shared_ptr<Volume> Fresh(int main_blocks, int excess_blocks)
{
  auto volume = std::make_shared<Volume>(main_blocks, excess_blocks);
  volume->SetVoxelLength(0.008f);
  return volume;
}

static std::shared_ptr<Volume> Fused(int main_blocks, int excess_blocks, const Frame& frame, int integrations)
{
  auto volume = Fresh(main_blocks, excess_blocks);
  for (int i = 0; i < 6; ++i) volume->SetView(frame);
  DepthIntegrator integrator(volume);
  for (int i = 0; i < integrations; ++i) integrator.Integrate(frame);
  return volume;
}

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

int main(int argc, char** argv)
{
  int count = 0;
  VK_ASSERT(vk_device_count(&count));
  if (count == 0) { std::printf("register_tests: no HIP device\n"); return 2; }
  const std::string filter = argc > 1 ? argv[1] : "";
  int failed = 0, ran = 0;
  for (const TestCase& t : Registry())
  {
    if (!filter.empty() && std::string(t.name).find(filter) == std::string::npos) continue;
    ++ran;
    try { t.body(); Device::Synchronize(); std::printf("[  OK  ] %s\n", t.name); }
    catch (const Failure& f) { ++failed; std::printf("[FAILED] %s\n         %s\n", t.name, f.text.c_str()); }
    catch (const std::exception& e) { ++failed; std::printf("[FAILED] %s\n         exception: %s\n", t.name, e.what()); }
    std::fflush(stdout);
  }
  std::printf("%d test(s), %d failed\n", ran, failed);
  return failed ? 1 : 0;
}
