// volume_test_support.h — what the test programs of the volume operations share (release, merge, merge_pose, register,
// sample, cast, integrate_rays and mesh_attribute _tests.cpp): the harness of host_tests.cpp (TEST, the ASSERT_ macros, the
// runner that main calls) and the scenes and read-backs several of them use. A bound that differs between programs
// (kDepthBound) stays with its program.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
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
inline std::vector<TestCase>& Registry() { static std::vector<TestCase> r; return r; }
struct Registrar { Registrar(const char* n, std::function<void()> f) { Registry().push_back({n, f}); } };
#define TEST(suite, name) static void suite##_##name(); \
    static Registrar reg_##suite##_##name(#suite "." #name, suite##_##name); static void suite##_##name()

// main: every case, or the cases whose name contains argv[1]; "[  OK  ] Name" per case, then "N test(s), M failed"
inline int RunTests(const char* program, int argc, char** argv)
{
  int count = 0;
  VK_ASSERT(vk_device_count(&count));
  if (count == 0) { std::printf("%s: no HIP device\n", program); return 2; }
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

static const int kWidth = 160, kHeight = 120;
static const float kVoxel = 0.008f;

inline std::shared_ptr<Image> MakeDepth(const std::function<float(int, int)>& f)
{
  std::vector<float> host(size_t(kWidth) * kHeight);
  for (int y = 0; y < kHeight; ++y) for (int x = 0; x < kWidth; ++x) host[size_t(y) * kWidth + x] = f(x, y);
  auto image = std::make_shared<Image>(kWidth, kHeight);
  image->CopyFromHost(host.data());
  return image;
}

// the camera every scene is seen through, at `pose`
inline Frame DepthFrame(const std::function<float(int, int)>& depth, const Transform& pose)
{
  Frame frame;
  frame.depth_projection.SetFocalLength(136, 136);
  frame.depth_projection.SetCenterPoint(80, 60);
  frame.depth_image = MakeDepth(depth);
  frame.depth_to_world_transform = pose;
  return frame;
}

// a slanted wall at 1.5 m
inline Frame SlantedFrame(const Transform& pose)
{
  return DepthFrame([](int x, int y) { return 1.5f + 0.001f * x + 0.0007f * y; }, pose);
}

// the scene of tests/register_reference.py: a wall at 1 m with a bump, a dent and a slope — nothing repeats and no direction
// is free, so an alignment has one answer
inline float Bumps(int x, int y)
{
  const double w = kWidth, h = kHeight;
  const double bump = std::exp(-((x - 0.375 * w) * (x - 0.375 * w) + (y - 0.42 * h) * (y - 0.42 * h)) / (2 * (0.16 * w) * (0.16 * w)));
  const double dent = std::exp(-((x - 0.69 * w) * (x - 0.69 * w) + (y - 0.67 * h) * (y - 0.67 * h)) / (2 * (0.11 * w) * (0.11 * w)));
  return float(1.0 + 0.06 * bump - 0.04 * dent + 0.03 * x / w);
}

inline Frame BumpsFrame(const Transform& pose) { return DepthFrame(Bumps, pose); }

inline std::shared_ptr<Volume> Fresh(int main_blocks, int excess_blocks)
{
  auto volume = std::make_shared<Volume>(main_blocks, excess_blocks);
  volume->SetVoxelLength(kVoxel);
  return volume;
}

inline std::shared_ptr<Volume> Fused(int main_blocks, int excess_blocks, const Frame& frame, int integrations)
{
  auto volume = Fresh(main_blocks, excess_blocks);
  for (int i = 0; i < 6; ++i) volume->SetView(frame);
  DepthIntegrator integrator(volume);
  for (int i = 0; i < integrations; ++i) integrator.Integrate(frame);
  return volume;
}

inline std::vector<vk_hash_entry> Entries(const Volume& volume)
{
  const vk_volume v = volume.ToVk();
  std::vector<vk_hash_entry> host(size_t(v.main_block_count) + v.excess_block_count);
  VK_ASSERT(vk_memcpy_d2h(host.data(), v.hash_entries, sizeof(vk_hash_entry) * host.size(), Device::GetStream()));
  return host;
}

inline std::vector<vk_voxel> Voxels(const Volume& volume)
{
  const vk_volume v = volume.ToVk();
  std::vector<vk_voxel> host((size_t(v.main_block_count) + v.excess_block_count) * VK_BLOCK_VOXELS);
  VK_ASSERT(vk_memcpy_d2h(host.data(), v.voxels, sizeof(vk_voxel) * host.size(), Device::GetStream()));
  return host;
}

// the 512 voxels of every block, by origin
typedef std::map<std::array<int16_t, 3>, const vk_voxel*> BlockMap;
inline BlockMap Blocks(const std::vector<vk_hash_entry>& entries, const std::vector<vk_voxel>& voxels)
{
  BlockMap out;
  for (const vk_hash_entry& e : entries)
    if (e.data >= 0) out[{{e.block.origin[0], e.block.origin[1], e.block.origin[2]}}] = voxels.data() + size_t(e.data) * VK_BLOCK_VOXELS;
  return out;
}

// the pixel rays of the frame's camera, in the camera's frame: from its centre through every pixel's centre
inline std::vector<Ray> PixelRays(const Frame& frame)
{
  std::vector<Ray> rays(size_t(kWidth) * kHeight);
  for (int y = 0; y < kHeight; ++y)
    for (int x = 0; x < kWidth; ++x)
    {
      Ray& ray = rays[size_t(y) * kWidth + x];
      ray.origin = Vector3f(0.0f, 0.0f, 0.0f);
      ray.direction = frame.depth_projection.Unproject(x + 0.5f, y + 0.5f);
    }
  return rays;
}

inline float Length(const Vector3f& v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
