// merge_resampled_bad_arguments.cpp — every refusal of the host checks of vk_volume_merge_resampled and
// vk_volume_merge_resampled_workspace_bytes (include/vk.h), with addresses that are no memory: a stand-alone program for a
// host sanitizer run of those checks. No GPU is needed or touched: each call has to return VK_ERR_ARGUMENT before anything
// is enqueued. Build it with the entry points' own source, the rest of the library as it is:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -I include -I vulcan_amd/csrc -I tools/debug vulcan_amd/csrc/vk_merge_resample.hip tools/debug/merge_resampled_bad_arguments.cpp \
//     -L vulcan_amd/lib -lvk_hip -Wl,-rpath,$PWD/vulcan_amd/lib -o merge_resampled_bad_arguments
#include "bad_arguments.h"

static vk_transform Identity()
{
  vk_transform t = {};
  for (int a = 0; a < 4; ++a) t.m[5 * a] = t.inv[5 * a] = 1.0f;
  return t;
}

static vk_merge_resample_params Params(int supersample = 1, int reserved = 0, int flags = 0, int max_rounds = 8, float cap_d = 16.0f,
    float cap_c = 16.0f)
{
  vk_merge_resample_params p = {};
  p.merge.flags = flags;
  p.merge.max_rounds = max_rounds;
  p.merge.max_distance_weight = cap_d;
  p.merge.max_color_weight = cap_c;
  p.pose = Identity();
  p.supersample = supersample;
  p.reserved = reserved;
  return p;
}

static int Merge(const vk_volume* dst, const vk_volume* src, const vk_merge_resample_params* p, int32_t* counts = kInts,
    void* workspace = kWorkspace)
{
  return vk_volume_merge_resampled(dst, src, p, counts, workspace, nullptr);
}

// the source volume at other lengths
static vk_volume Source(float voxel_length = 0.008f, float truncation_length = 0.04f)
{
  vk_volume v = Volume(uintptr_t(2) << 20);
  v.voxel_length = voxel_length;
  v.truncation_length = truncation_length;
  return v;
}

int main()
{
  static_assert(sizeof(vk_merge_resample_params) == 16 + 128 + 8, "vk_merge_params, vk_transform, two words");
  const vk_volume dst = Volume(), src = Source();
  const vk_merge_resample_params p = Params();
  EXPECT(VK_ERR_ARGUMENT, Merge(nullptr, &src, &p));
  EXPECT(VK_ERR_ARGUMENT, Merge(&dst, nullptr, &p));
  EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &p, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &p, kInts, nullptr));
  EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &dst, &p));                      // into itself
  {
    vk_volume broken = Source();
    broken.hash_entries = nullptr;
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &broken, &p));
    EXPECT(VK_ERR_ARGUMENT, Merge(&broken, &src, &p));
    broken = Source();
    broken.main_block_count = 0;
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &broken, &p));
    broken = Source();
    broken.excess_block_count = kMost;
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &broken, &p));
    broken = Volume((uintptr_t(2) << 20) + 8);                         // a pool that is not 16-byte aligned
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &broken, &p));
  }
  // the ratio of the voxel lengths, either way round, lies in [0.25, 4]
  const float lengths[] = {0.0f, -0.008f, kNan, kInf, 0.008f * 0.2f, 0.008f * 0.2499f, 0.008f * 4.001f, 0.008f * 4.5f, 1e-30f, 1e30f};
  for (float length : lengths)
  {
    const vk_volume other = Source(length);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &other, &p));
    EXPECT(VK_ERR_ARGUMENT, Merge(&other, &dst, &p));
  }
  // the ratio of the truncation lengths is finite and > 0
  const float truncations[] = {0.0f, -0.04f, kNan, kInf, -kInf};
  for (float truncation : truncations)
  {
    const vk_volume other = Source(0.008f, truncation);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &other, &p));
    EXPECT(VK_ERR_ARGUMENT, Merge(&other, &dst, &p));
  }
  {
    const vk_volume tiny = Source(0.008f, 1e-38f), huge = Source(0.008f, 1e38f);     // each a volume; the quotient is not finite, or 0
    EXPECT(VK_ERR_ARGUMENT, Merge(&tiny, &huge, &p));
    EXPECT(VK_ERR_ARGUMENT, Merge(&huge, &tiny, &p));
  }
  const int supersamples[] = {0, -1, 5, 64, kMost, kLeast};
  for (int n : supersamples)
  {
    const vk_merge_resample_params bad = Params(n);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad));
  }
  const int reserved[] = {1, -1, kMost, kLeast};
  for (int word : reserved)
  {
    const vk_merge_resample_params bad = Params(1, word);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad));
  }
  const int flags[] = {4, 8, -1, 1 << 16, kLeast};
  for (int f : flags)
  {
    const vk_merge_resample_params bad = Params(1, 0, f);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad));
  }
  const int rounds[] = {0, -1, kLeast};
  for (int n : rounds)
  {
    const vk_merge_resample_params bad = Params(1, 0, 0, n);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad));
  }
  const float caps[] = {0.0f, 0.5f, -1.0f, 32768.0f, kInf, kNan};
  for (float cap : caps)
  {
    const vk_merge_resample_params bad_d = Params(1, 0, 0, 8, cap), bad_c = Params(1, 0, 0, 8, 16.0f, cap);
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad_d));
    EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad_c));
  }
  // rows 0-2 of the matrix and of its inverse are finite
  const int entries[] = {0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14};
  const float bad_values[] = {kNan, kInf, -kInf};
  for (int at : entries)
    for (float value : bad_values)
    {
      vk_merge_resample_params bad = Params();
      bad.pose.m[at] = value;
      EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad));
      bad = Params();
      bad.pose.inv[at] = value;
      EXPECT(VK_ERR_ARGUMENT, Merge(&dst, &src, &bad));
    }
  // the workspace: sizes that are a volume's and a box of 2 .. 8 blocks per axis
  const int32_t sizes[][4] = {{0, 8, 8, 8}, {-1, 8, 8, 8}, {8, -1, 8, 8}, {8, 8, 0, 8}, {8, 8, 8, -1}, {kMost, 1, 8, 8}, {8, 8, kMost, kMost},
      {kLeast, 8, 8, 8}};
  for (const auto& s : sizes) EXPECT(0, vk_volume_merge_resampled_workspace_bytes(s[0], s[1], s[2], s[3], 3) != 0);
  const int32_t boxes[] = {1, 0, -1, 9, kMost, kLeast};
  for (int32_t box : boxes) EXPECT(0, vk_volume_merge_resampled_workspace_bytes(8, 8, 8, 8, box) != 0);
  for (int32_t box = 2; box <= 8; ++box) EXPECT(1, vk_volume_merge_resampled_workspace_bytes(8, 8, 8, 8, box) >= size_t(16) * (33 + 4 * ((box * box * box + 31) / 32)));
  EXPECT(1, vk_volume_merge_resampled_workspace_bytes(kMost - 8, 8, kMost - 8, 8, 8) > size_t(kMost) * 64);
  return Finish("merge_resampled_bad_arguments");
}
