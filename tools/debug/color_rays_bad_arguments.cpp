// color_rays_bad_arguments.cpp — every refusal of vk_volume_color_rays' host checks (include/vk.h), with addresses that are
// no memory: a stand-alone program for a host sanitizer run of those checks. No GPU is needed or touched: each call has to
// return VK_ERR_ARGUMENT (or 0 for count == 0) before anything is enqueued. Build it with the entry point's own source, the
// rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc -I tools/debug vulcan_amd/csrc/vk_color_rays.hip tools/debug/color_rays_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o color_rays_bad_arguments
#include "bad_arguments.h"

static vk_color_rays_params Params(int flags = 0, float r_min = 0.1f, float r_max = 5.0f, float band = 0.04f, float cap = 16.0f)
{
  vk_color_rays_params p = {};
  p.flags = flags;
  p.r_min = r_min;
  p.r_max = r_max;
  p.band = band;
  p.max_color_weight = cap;
  return p;
}

int main()
{
  static_assert(sizeof(vk_color_rays_params) == 24, "vk_color_rays_params");
  const float* rays = kRays;
  int32_t* counts = kInts;
  void* workspace = kWorkspace;
  const vk_volume v = Volume();
  const vk_color_rays_params p = Params();
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(nullptr, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, nullptr, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &p, nullptr, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &p, counts, nullptr, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &p, counts, static_cast<char*>(workspace) + 8, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, nullptr, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, nullptr, rays, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, nullptr, 8, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, -1, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, (1 << 21) + 1, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 1 << 22, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, kMost, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, kLeast, nullptr, &p, counts, workspace, nullptr));
  {
    vk_volume broken = Volume();
    broken.hash_entries = nullptr;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.voxel_length = 0.0f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.main_block_count = 0;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.excess_block_count = kMost;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume((uintptr_t(1) << 20) + 8);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.truncation_length = 0.008f * 64.5f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken.truncation_length = kNan;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    // the band is measured in this volume's voxels: what passes at 8 mm does not at 0.5 mm
    broken = Volume();
    broken.voxel_length = 0.0005f;
    broken.truncation_length = 0.0025f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
  }
  const int flags[] = {4, 7, 8, -1, 1 << 16, kLeast};
  for (int f : flags)
  {
    const vk_color_rays_params bad = Params(f);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float caps[] = {0.5f, 0.0f, -1.0f, 32768.0f, kInf, kNan};
  for (float c : caps)
  {
    const vk_color_rays_params bad = Params(0, 0.1f, 5.0f, 0.04f, c);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float bounds[][2] = {{-0.001f, 5.0f}, {1.0f, 1.0f}, {2.0f, 1.0f}, {0.0f, kInf}, {0.0f, kNan}, {kNan, 5.0f}, {-kInf, 5.0f}, {0.0f, 0.0f}};
  for (const auto& b : bounds)
  {
    const vk_color_rays_params bad = Params(0, b[0], b[1]);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float bands[] = {0.0f, -0.0f, -0.001f, -kInf, kInf, kNan, 0.008f * 64.5f, 1e30f};
  for (float b : bands)
  {
    const vk_color_rays_params bad = Params(0, 0.1f, 5.0f, b);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  {
    const vk_color_rays_params bad = Params(VK_RAYS_VOXEL_UNITS, 0.1f, 5.0f, 64.5f);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  // count == 0 launches nothing but is checked like any call
  EXPECT(VK_OK, vk_volume_color_rays(&v, nullptr, nullptr, nullptr, 0, nullptr, &p, counts, workspace, nullptr));
  EXPECT(VK_OK, vk_volume_color_rays(&v, rays, rays, rays, 0, nullptr, &p, counts, workspace, nullptr));
  {
    const vk_color_rays_params widest = Params(3, 0.0f, 1e30f, 64.0f, 32767.0f);
    EXPECT(VK_OK, vk_volume_color_rays(&v, rays, rays, rays, 0, nullptr, &widest, counts, workspace, nullptr));
    const vk_color_rays_params least = Params(0, 0.0f, 1e-30f, 1e-30f, 1.0f);
    EXPECT(VK_OK, vk_volume_color_rays(&v, rays, rays, rays, 0, nullptr, &least, counts, workspace, nullptr));
  }
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 0, nullptr, &p, nullptr, workspace, nullptr));
  {
    const vk_color_rays_params bad = Params(0, 0.1f, 5.0f, 0.0f);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 0, nullptr, &bad, counts, workspace, nullptr));
  }
  // the pass events: five, none of them null, or (null, 0)
  void* events[5] = {workspace, workspace, workspace, nullptr, workspace};
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays_time_next(events, 5));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays_time_next(events, 4));
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays_time_next(nullptr, 5));
  EXPECT(VK_OK, vk_volume_color_rays_time_next(nullptr, 0));
  EXPECT(0, vk_volume_color_rays_workspace_bytes(0, 0) != 0);
  EXPECT(0, vk_volume_color_rays_workspace_bytes(8, -1) != 0);
  EXPECT(0, vk_volume_color_rays_workspace_bytes(kMost, kMost) != 0);
  EXPECT(1, vk_volume_color_rays_workspace_bytes(509, 96) >= size_t(605) * (512 * 16 + 1));
  return Finish("color_rays_bad_arguments");
}
