// score_poses_bad_arguments.cpp — every refusal of the host checks of vk_volume_score_poses, vk_volume_score_poses_best and
// vk_volume_score_poses_workspace_bytes (include/vk.h), with addresses that are no memory: a stand-alone program for a host
// sanitizer run of those checks. No GPU is needed or touched: each call has to return VK_ERR_ARGUMENT (or 0 for count == 0)
// before anything is enqueued. Build it with the entry points' own source, the rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc -I tools/debug vulcan_amd/csrc/vk_score_poses.hip tools/debug/score_poses_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o score_poses_bad_arguments
#include "bad_arguments.h"

static vk_score_poses_params Params(int flags = 0, int min_residuals = 1, float r_min = 0.1f, float r_max = 5.0f, float band = 0.75f)
{
  vk_score_poses_params p = {};
  p.flags = flags;
  p.min_residuals = min_residuals;
  p.r_min = r_min;
  p.r_max = r_max;
  p.max_abs_distance = band;
  return p;
}

static vk_pose_score* const kScores = reinterpret_cast<vk_pose_score*>(uintptr_t(28672));
static vk_transform* const kPoses = kPose;

static int Score(const vk_volume* v, const float* rays, const float* ranges, int32_t count, const vk_transform* poses, int32_t pose_count,
    const vk_score_poses_params* p, vk_pose_score* scores = kScores, void* workspace = kWorkspace)
{
  return vk_volume_score_poses(v, rays, ranges, count, poses, pose_count, p, scores, workspace, nullptr);
}

int main()
{
  static_assert(sizeof(vk_score_poses_params) == 24 && sizeof(vk_pose_score) == 32, "the two structs");
  const vk_volume v = Volume();
  const vk_score_poses_params p = Params();
  EXPECT(VK_ERR_ARGUMENT, Score(nullptr, kRays, kRays, 8, kPoses, 8, &p));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, nullptr, 8, &p));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &p, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &p, kScores, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &p, kScores, static_cast<char*>(kWorkspace) + 8));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, nullptr, kRays, 8, kPoses, 8, &p));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, nullptr, 8, kPoses, 8, &p));
  const int32_t counts[] = {-1, (1 << 22) + 1, kMost, kLeast};
  for (int32_t n : counts) EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, n, kPoses, 1, &p));
  const int32_t pose_counts[] = {0, -1, 65537, kMost, kLeast};
  for (int32_t n : pose_counts)
  {
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, n, &p));
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 0, kPoses, n, &p));
    EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, kPoses, n, &p, kInts, kPoses, nullptr));
    EXPECT(0, vk_volume_score_poses_workspace_bytes(8, n) != 0);
  }
  // the product: 1 << 28 pairs are the kMost
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 1 << 22, kPoses, 65, &p));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, (1 << 12) + 1, kPoses, 65536, &p));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, (1 << 14) + 1, kPoses, 1 << 14, &p));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 1 << 22, kPoses, 65536, &p));
  {
    vk_volume broken = Volume();
    broken.hash_entries = nullptr;
    EXPECT(VK_ERR_ARGUMENT, Score(&broken, kRays, kRays, 8, kPoses, 8, &p));
    broken = Volume();
    broken.voxel_length = 0.0f;
    EXPECT(VK_ERR_ARGUMENT, Score(&broken, kRays, kRays, 8, kPoses, 8, &p));
    broken = Volume();
    broken.truncation_length = kNan;
    EXPECT(VK_ERR_ARGUMENT, Score(&broken, kRays, kRays, 8, kPoses, 8, &p));
    broken = Volume();
    broken.main_block_count = 0;
    EXPECT(VK_ERR_ARGUMENT, Score(&broken, kRays, kRays, 8, kPoses, 8, &p));
    broken = Volume();
    broken.excess_block_count = kMost;
    EXPECT(VK_ERR_ARGUMENT, Score(&broken, kRays, kRays, 8, kPoses, 8, &p));
    broken = Volume((uintptr_t(1) << 20) + 8);
    EXPECT(VK_ERR_ARGUMENT, Score(&broken, kRays, kRays, 8, kPoses, 8, &p));
  }
  const int flags[] = {2, 3, 4, 8, -1, 1 << 16, kLeast};
  for (int f : flags)
  {
    const vk_score_poses_params bad = Params(f);
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &bad));
    EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, kPoses, 8, &bad, kInts, kPoses, nullptr));
  }
  const int fewest[] = {0, -1, kLeast};
  for (int n : fewest)
  {
    const vk_score_poses_params bad = Params(0, n);
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &bad));
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 0, kPoses, 8, &bad));
    EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, kPoses, 8, &bad, kInts, kPoses, nullptr));
  }
  const float bounds[][2] = {{-0.001f, 5.0f}, {1.0f, 1.0f}, {2.0f, 1.0f}, {0.0f, kInf}, {0.0f, kNan}, {kNan, 5.0f}, {-kInf, 5.0f}, {0.0f, 0.0f}};
  for (const auto& b : bounds)
  {
    const vk_score_poses_params bad = Params(0, 1, b[0], b[1]);
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &bad));
  }
  const float bands[] = {0.0f, -0.0f, -0.5f, 1.0000001f, 1.5f, kInf, -kInf, kNan};
  for (float b : bands)
  {
    const vk_score_poses_params bad = Params(0, 1, 0.1f, 5.0f, b);
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 8, kPoses, 8, &bad));
    EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 0, kPoses, 8, &bad));
  }
  // vk_volume_score_poses_best: every pointer is needed
  EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(nullptr, kPoses, 8, &p, kInts, kPoses, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, nullptr, 8, &p, kInts, kPoses, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, kPoses, 8, nullptr, kInts, kPoses, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, kPoses, 8, &p, nullptr, kPoses, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_score_poses_best(kScores, kPoses, 8, &p, kInts, nullptr, nullptr));
  // count == 0 launches nothing but is checked like any call
  EXPECT(VK_OK, Score(&v, nullptr, nullptr, 0, kPoses, 8, &p));
  EXPECT(VK_OK, Score(&v, kRays, kRays, 0, kPoses, 1, &p));
  EXPECT(VK_OK, Score(&v, kRays, kRays, 0, kPoses, 65536, &p));
  {
    const vk_score_poses_params widest = Params(VK_RAYS_VOXEL_UNITS, kMost, 0.0f, 1e30f, 1.0f);
    EXPECT(VK_OK, Score(&v, kRays, kRays, 0, kPoses, 8, &widest));
    const vk_score_poses_params narrowest = Params(0, 1, 0.0f, 1e-30f, 1e-30f);
    EXPECT(VK_OK, Score(&v, kRays, kRays, 0, kPoses, 8, &narrowest));
  }
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 0, nullptr, 8, &p));
  {
    vk_volume wide = Volume();                      // nothing walks a band: the 64 voxels of the walks' truncation bound are none here
    wide.truncation_length = 0.008f * 64.5f;
    EXPECT(VK_OK, Score(&wide, kRays, kRays, 0, kPoses, 8, &p));
  }
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 0, kPoses, 8, &p, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Score(&v, kRays, kRays, 0, kPoses, 8, &p, kScores, nullptr));
  for (int32_t n : counts) EXPECT(0, vk_volume_score_poses_workspace_bytes(n, 1) != 0);
  EXPECT(0, vk_volume_score_poses_workspace_bytes(1 << 22, 65) != 0);
  EXPECT(0, vk_volume_score_poses_workspace_bytes(kMost, kMost) != 0);
  EXPECT(1, vk_volume_score_poses_workspace_bytes(0, 1) >= 32);
  EXPECT(1, vk_volume_score_poses_workspace_bytes(1 << 22, 64) == (size_t(1) << 14) * 64 * 32);
  EXPECT(1, vk_volume_score_poses_workspace_bytes(1 << 12, 65536) == size_t(16) * 65536 * 32);
  EXPECT(1, vk_volume_score_poses_workspace_bytes(257, 3) >= size_t(2) * 3 * 32);
  return Finish("score_poses_bad_arguments");
}
