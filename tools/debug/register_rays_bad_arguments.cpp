// register_rays_bad_arguments.cpp — every refusal of the host checks of vk_volume_register_rays, vk_volume_register_rays_system
// and vk_volume_register_rays_terms (include/vk.h), with addresses that are no memory: a stand-alone program for a host
// sanitizer run of those checks. No GPU is needed or touched: each call has to return VK_ERR_ARGUMENT (or 0 for count == 0)
// before anything is enqueued. Build it with the entry points' own source, the rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc -I tools/debug vulcan_amd/csrc/vk_register_rays.hip tools/debug/register_rays_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o register_rays_bad_arguments
#include "bad_arguments.h"

static vk_register_rays_params Params(int flags = 0, int iterations = 20, float r_min = 0.1f, float r_max = 5.0f, float band = 0.75f)
{
  vk_register_rays_params p = {};
  p.flags = flags;
  p.iterations = iterations;
  p.r_min = r_min;
  p.r_max = r_max;
  p.max_abs_distance = band;
  return p;
}

// the three entry points with the arguments they share: whatever one refuses for them, all three refuse
static void All(int code, const vk_volume* v, const float* rays, const float* ranges, int32_t count, vk_transform* pose,
    const vk_register_rays_params* p, void* workspace, int line)
{
  const int got[3] = {vk_volume_register_rays(v, rays, ranges, count, pose, p, kFloats, kInts, kInts, kFloats, workspace, nullptr),
      vk_volume_register_rays_system(v, rays, ranges, count, pose, p, kFloats, kInts, workspace, nullptr),
      vk_volume_register_rays_terms(v, rays, ranges, count, pose, p, kFloats, kFloats, kBytes, workspace, nullptr)};
  for (int k = 0; k < 3; ++k)
    if (got[k] != code)
    {
      ++g_failed;
      std::printf("line %d: entry point %d: expected %d, got %d\n", line, k, code, got[k]);
    }
}
#define ALL(code, ...) All((code), __VA_ARGS__, __LINE__)

int main()
{
  static_assert(sizeof(vk_register_rays_params) == 24, "vk_register_rays_params");
  const vk_volume v = Volume();
  const vk_register_rays_params p = Params();
  ALL(VK_ERR_ARGUMENT, nullptr, kRays, kRays, 8, kPose, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, nullptr, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, nullptr, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, &p, nullptr);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, &p, static_cast<char*>(kWorkspace) + 8);
  ALL(VK_ERR_ARGUMENT, &v, nullptr, kRays, 8, kPose, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, nullptr, 8, kPose, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, -1, kPose, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, (1 << 22) + 1, kPose, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, kMost, kPose, &p, kWorkspace);
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, kLeast, kPose, &p, kWorkspace);
  {
    vk_volume broken = Volume();
    broken.hash_entries = nullptr;
    ALL(VK_ERR_ARGUMENT, &broken, kRays, kRays, 8, kPose, &p, kWorkspace);
    broken = Volume();
    broken.voxel_length = 0.0f;
    ALL(VK_ERR_ARGUMENT, &broken, kRays, kRays, 8, kPose, &p, kWorkspace);
    broken = Volume();
    broken.truncation_length = kNan;
    ALL(VK_ERR_ARGUMENT, &broken, kRays, kRays, 8, kPose, &p, kWorkspace);
    broken = Volume();
    broken.main_block_count = 0;
    ALL(VK_ERR_ARGUMENT, &broken, kRays, kRays, 8, kPose, &p, kWorkspace);
    broken = Volume();
    broken.excess_block_count = kMost;
    ALL(VK_ERR_ARGUMENT, &broken, kRays, kRays, 8, kPose, &p, kWorkspace);
    broken = Volume((uintptr_t(1) << 20) + 8);
    ALL(VK_ERR_ARGUMENT, &broken, kRays, kRays, 8, kPose, &p, kWorkspace);
  }
  const int flags[] = {2, 3, 4, 8, -1, 1 << 16, kLeast};
  for (int f : flags)
  {
    const vk_register_rays_params bad = Params(f);
    ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, &bad, kWorkspace);
  }
  const int steps[] = {0, -1, 65, kMost, kLeast};
  for (int n : steps)
  {
    const vk_register_rays_params bad = Params(0, n);
    ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, &bad, kWorkspace);
  }
  const float bounds[][2] = {{-0.001f, 5.0f}, {1.0f, 1.0f}, {2.0f, 1.0f}, {0.0f, kInf}, {0.0f, kNan}, {kNan, 5.0f}, {-kInf, 5.0f}, {0.0f, 0.0f}};
  for (const auto& b : bounds)
  {
    const vk_register_rays_params bad = Params(0, 20, b[0], b[1]);
    ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, &bad, kWorkspace);
  }
  const float bands[] = {0.0f, -0.0f, -0.5f, 1.0000001f, 1.5f, kInf, -kInf, kNan};
  for (float b : bands)
  {
    const vk_register_rays_params bad = Params(0, 20, 0.1f, 5.0f, b);
    ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 8, kPose, &bad, kWorkspace);
  }
  // an output of its own that each entry point needs (update_dev alone may be null)
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays(&v, kRays, kRays, 8, kPose, &p, nullptr, kInts, kInts, kFloats, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays(&v, kRays, kRays, 8, kPose, &p, kFloats, nullptr, kInts, kFloats, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays(&v, kRays, kRays, 8, kPose, &p, kFloats, kInts, nullptr, kFloats, kWorkspace, nullptr));
  EXPECT(VK_OK, vk_volume_register_rays(&v, kRays, kRays, 0, kPose, &p, kFloats, kInts, kInts, nullptr, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays_system(&v, kRays, kRays, 8, kPose, &p, nullptr, kInts, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays_system(&v, kRays, kRays, 8, kPose, &p, kFloats, nullptr, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays_terms(&v, kRays, kRays, 8, kPose, &p, nullptr, kFloats, kBytes, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays_terms(&v, kRays, kRays, 8, kPose, &p, kFloats, nullptr, kBytes, kWorkspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_register_rays_terms(&v, kRays, kRays, 8, kPose, &p, kFloats, kFloats, nullptr, kWorkspace, nullptr));
  // count == 0 launches nothing but is checked like any call
  ALL(VK_OK, &v, nullptr, nullptr, 0, kPose, &p, kWorkspace);
  ALL(VK_OK, &v, kRays, kRays, 0, kPose, &p, kWorkspace);
  {
    const vk_register_rays_params widest = Params(VK_RAYS_VOXEL_UNITS, 64, 0.0f, 1e30f, 1.0f);
    ALL(VK_OK, &v, kRays, kRays, 0, kPose, &widest, kWorkspace);
    const vk_register_rays_params least = Params(0, 1, 0.0f, 1e-30f, 1e-30f);
    ALL(VK_OK, &v, kRays, kRays, 0, kPose, &least, kWorkspace);
    const vk_register_rays_params bad = Params(0, 20, 0.1f, 5.0f, 0.0f);
    ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 0, kPose, &bad, kWorkspace);
  }
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 0, nullptr, &p, kWorkspace);
  {
    vk_volume wide = Volume();                      // nothing walks a band: the 64 voxels of the walks' truncation bound are none here
    wide.truncation_length = 0.008f * 64.5f;
    ALL(VK_OK, &wide, kRays, kRays, 0, kPose, &p, kWorkspace);
  }
  ALL(VK_ERR_ARGUMENT, &v, kRays, kRays, 0, kPose, &p, nullptr);
  EXPECT(0, vk_volume_register_rays_workspace_bytes(-1) != 0);
  EXPECT(0, vk_volume_register_rays_workspace_bytes((1 << 22) + 1) != 0);
  EXPECT(0, vk_volume_register_rays_workspace_bytes(kMost) != 0);
  EXPECT(0, vk_volume_register_rays_workspace_bytes(kLeast) != 0);
  EXPECT(1, vk_volume_register_rays_workspace_bytes(0) >= 128);
  EXPECT(1, vk_volume_register_rays_workspace_bytes(1 << 22) >= size_t(4096) * 128);
  return Finish("register_rays_bad_arguments");
}
