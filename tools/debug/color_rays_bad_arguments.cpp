// color_rays_bad_arguments.cpp — every refusal of vk_volume_color_rays' host checks (include/vk.h), with addresses that are
// no memory: a stand-alone program for a host sanitizer run of those checks. No GPU is needed or touched: each call has to
// return VK_ERR_ARGUMENT (or 0 for count == 0) before anything is enqueued. Build it with the entry point's own source, the
// rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc vulcan_amd/csrc/vk_color_rays.hip tools/debug/color_rays_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o color_rays_bad_arguments
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "vk.h"

static int g_failed = 0;
#define EXPECT(code, call) do { const int got__ = (call); if (got__ != (code)) { ++g_failed; \
    std::printf("line %d: expected %d, got %d: %s\n", __LINE__, (code), got__, #call); } } while (0)

static vk_volume Volume(uintptr_t base = uintptr_t(1) << 20)
{
  vk_volume v = {};
  void** fields[8] = {reinterpret_cast<void**>(&v.voxels), reinterpret_cast<void**>(&v.hash_entries), reinterpret_cast<void**>(&v.free_voxel_blocks),
      reinterpret_cast<void**>(&v.allocation_types), reinterpret_cast<void**>(&v.allocation_blocks), reinterpret_cast<void**>(&v.block_visibility),
      reinterpret_cast<void**>(&v.visible_blocks), reinterpret_cast<void**>(&v.counters)};
  for (int k = 0; k < 8; ++k) *fields[k] = reinterpret_cast<void*>(base + 4096 * uintptr_t(k));
  v.main_block_count = 8;
  v.excess_block_count = 8;
  v.voxel_length = 0.008f;
  v.truncation_length = 0.04f;
  return v;
}

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
  const float* rays = reinterpret_cast<const float*>(uintptr_t(4096));
  int32_t* counts = reinterpret_cast<int32_t*>(uintptr_t(8192));
  void* workspace = reinterpret_cast<void*>(uintptr_t(16384));
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
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
  EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, std::numeric_limits<int32_t>::max(), nullptr, &p, counts, workspace, nullptr));
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
    broken.excess_block_count = std::numeric_limits<int32_t>::max();
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume((uintptr_t(1) << 20) + 8);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken = Volume();
    broken.truncation_length = 0.008f * 64.5f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    broken.truncation_length = nan;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
    // the band is measured in this volume's voxels: what passes at 8 mm does not at 0.5 mm
    broken = Volume();
    broken.voxel_length = 0.0005f;
    broken.truncation_length = 0.0025f;
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&broken, rays, rays, rays, 8, nullptr, &p, counts, workspace, nullptr));
  }
  const int flags[] = {4, 7, 8, -1, 1 << 16, std::numeric_limits<int32_t>::min()};
  for (int f : flags)
  {
    const vk_color_rays_params bad = Params(f);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float caps[] = {0.5f, 0.0f, -1.0f, 32768.0f, inf, nan};
  for (float c : caps)
  {
    const vk_color_rays_params bad = Params(0, 0.1f, 5.0f, 0.04f, c);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float bounds[][2] = {{-0.001f, 5.0f}, {1.0f, 1.0f}, {2.0f, 1.0f}, {0.0f, inf}, {0.0f, nan}, {nan, 5.0f}, {-inf, 5.0f}, {0.0f, 0.0f}};
  for (const auto& b : bounds)
  {
    const vk_color_rays_params bad = Params(0, b[0], b[1]);
    EXPECT(VK_ERR_ARGUMENT, vk_volume_color_rays(&v, rays, rays, rays, 8, nullptr, &bad, counts, workspace, nullptr));
  }
  const float bands[] = {0.0f, -0.0f, -0.001f, -inf, inf, nan, 0.008f * 64.5f, 1e30f};
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
  EXPECT(0, vk_volume_color_rays_workspace_bytes(std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::max()) != 0);
  EXPECT(1, vk_volume_color_rays_workspace_bytes(509, 96) >= size_t(605) * (512 * 16 + 1));
  std::printf("color_rays_bad_arguments: %d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
