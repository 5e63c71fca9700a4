// integrate_rays_bad_arguments.cpp — every refusal of vk_volume_integrate_rays' host checks (include/vk.h), with addresses
// that are no memory: a stand-alone program for a host sanitizer run of those checks. No GPU is needed or touched: each
// call has to return VK_ERR_ARGUMENT (or 0 for count == 0) before anything is enqueued. Build it with the entry point's own
// source, the rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc -I tools/debug vulcan_amd/csrc/vk_integrate_rays.hip tools/debug/integrate_rays_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o integrate_rays_bad_arguments
#include "bad_arguments.h"

static vk_integrate_rays_params Params(int flags = 0, int max_rounds = 8, float r_min = 0.1f, float r_max = 5.0f, float cap = 16.0f)
{
  vk_integrate_rays_params p = {};
  p.flags = flags;
  p.max_rounds = max_rounds;
  p.r_min = r_min;
  p.r_max = r_max;
  p.max_distance_weight = cap;
  return p;
}

int main()
{
  const float* rays = kRays;
  int32_t* counts = kInts;
  void* workspace = kWorkspace;
  const vk_volume v = Volume();
  const vk_integrate_rays_params p = Params();
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(nullptr, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, nullptr, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &p, nullptr, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &p, counts, nullptr, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &p, counts, static_cast<char*>(workspace) + 8, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, nullptr, rays, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, nullptr, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, -1, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, (1 << 22) + 1, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, kMost, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, kLeast, nullptr, &p, counts, workspace, nullptr));
  {
    vk_volume broken = Volume();
    broken.hash_entries = nullptr;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.voxel_length = 0.0f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.main_block_count = 0;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.excess_block_count = kMost;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume((uintptr_t(1) << 20) + 8);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.truncation_length = 0.008f * 64.5f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken.truncation_length = kNan;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&broken, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
  }
  const int flags[] = {4, 8, -1, 1 << 16, kLeast};
  for (int f : flags)
  {
    const vk_integrate_rays_params bad = Params(f);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const int rounds[] = {-1, 65, 1 << 30, kLeast};
  for (int r : rounds)
  {
    const vk_integrate_rays_params bad = Params(0, r);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float caps[] = {0.5f, 0.0f, -1.0f, 32768.0f, kInf, kNan};
  for (float c : caps)
  {
    const vk_integrate_rays_params bad = Params(0, 8, 0.1f, 5.0f, c);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float bounds[][2] = {{-0.001f, 5.0f}, {1.0f, 1.0f}, {2.0f, 1.0f}, {0.0f, kInf}, {0.0f, kNan}, {kNan, 5.0f}, {-kInf, 5.0f}, {0.0f, 0.0f}};
  for (const auto& b : bounds)
  {
    const vk_integrate_rays_params bad = Params(0, 8, b[0], b[1]);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  // count == 0 launches nothing but is checked like any call
  EXPECT(VK_OK, vk_volume_integrate_rays(&v, nullptr, nullptr, 0, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_OK, vk_volume_integrate_rays(&v, rays, rays, 0, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays(&v, rays, rays, 0, nullptr, &p, nullptr, workspace, nullptr));
  // the events of the measuring hook: six or none
  void* events[6] = {workspace, workspace, workspace, workspace, workspace, nullptr};
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays_time_next(events, 6));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays_time_next(events, 5));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_integrate_rays_time_next(nullptr, 6));
  EXPECT(VK_OK, vk_volume_integrate_rays_time_next(nullptr, 0));
  EXPECT(0, vk_volume_integrate_rays_workspace_bytes(0, 0) != 0);
  EXPECT(0, vk_volume_integrate_rays_workspace_bytes(8, -1) != 0);
  EXPECT(0, vk_volume_integrate_rays_workspace_bytes(kMost, kMost) != 0);
  EXPECT(1, vk_volume_integrate_rays_workspace_bytes(509, 96) >= size_t(605) * (512 * 12 + 1));
  return Finish("integrate_rays_bad_arguments");
}
