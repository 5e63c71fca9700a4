// merge_pose_tests.cpp — Volume::Merge(other, Tdst_src) through the C++ class layer -> C ABI -> HIP kernels (no upstream
// case: the reference's Volume is a process-wide singleton, src/volume.cu:17-21). The call's exact outcome is held against
// its CPU statement by tests/test_gpu_merge_pose.py; these cases are what a user of the class sees: at the identity pose
// the call is Merge(other), a translation by whole blocks into a fresh volume is a shifted copy, and a volume merged
// through a generic pose raycasts as the surface it was fused from. Harness: volume_test_support.h.
//
//   ./merge_pose_tests            run everything (needs a GPU)
//   ./merge_pose_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// the identity pose: every sample is the source voxel itself, the candidates are the source blocks
TEST(MergePose, IdentityIsThePlainMerge)
{
  const Frame left = SlantedFrame(Transform());
  const Frame right = SlantedFrame(Transform::Translate(0.3f, 0.0f, 0.0f));
  auto plain = Fused(8192, 2048, left, 2);
  auto posed = Fused(8192, 2048, left, 2);
  auto b = Fused(4093, 4096, right, 3);            // another table size
  const MergeCounts want = plain->Merge(*b);
  const MergePoseCounts got = posed->Merge(*b, Transform());
  ASSERT_EQ(want.considered, got.considered);
  ASSERT_EQ(want.considered, got.candidates);
  ASSERT_EQ(want.fused, got.fused);
  ASSERT_EQ(want.allocated, got.allocated);
  ASSERT_EQ(0, got.left_out);
  ASSERT_EQ(want.rounds, got.rounds);
  ASSERT_TRUE(got.sampled > 100000);
  const std::vector<vk_hash_entry> entries_plain = Entries(*plain), entries_posed = Entries(*posed);
  const std::vector<vk_voxel> voxels_plain = Voxels(*plain), voxels_posed = Voxels(*posed);
  ASSERT_TRUE(std::memcmp(entries_plain.data(), entries_posed.data(), sizeof(vk_hash_entry) * entries_plain.size()) == 0);
  ASSERT_TRUE(std::memcmp(voxels_plain.data(), voxels_posed.data(), sizeof(vk_voxel) * voxels_plain.size()) == 0);
  ASSERT_EQ(size_t(0), posed->GetVisibleBlocks().GetSize());        // until the next SetView
}

// a translation by (8, -16, 0) voxels into a fresh volume: the source's blocks, one block up in x and two down in y
TEST(MergePose, ABlockShiftIsAShiftedCopy)
{
  const Frame frame = SlantedFrame(Transform());
  auto source = Fused(509, 4096, frame, 2);        // long chains: several rounds
  auto fresh = std::make_shared<Volume>(1021, 2048);
  fresh->SetVoxelLength(0.008f);
  const int blocks = source->GetAllocatedBlockCount();
  MergeOptions options;
  options.max_rounds = 2;                          // the class layer goes on until every candidate has had its rounds
  const MergePoseCounts counts = fresh->Merge(*source, Transform::Translate(8.0f * 0.008f, -16.0f * 0.008f, 0.0f), options);
  ASSERT_EQ(blocks, counts.considered);
  ASSERT_EQ(blocks, counts.candidates);
  ASSERT_EQ(blocks, counts.fused);
  ASSERT_EQ(blocks, counts.allocated);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.rounds > 2);
  const std::vector<vk_hash_entry> entries_s = Entries(*source), entries_f = Entries(*fresh);
  const std::vector<vk_voxel> voxels_s = Voxels(*source), voxels_f = Voxels(*fresh);
  const BlockMap want = Blocks(entries_s, voxels_s), got = Blocks(entries_f, voxels_f);
  ASSERT_EQ(want.size(), got.size());
  for (const auto& block : want)
  {
    const std::array<int16_t, 3> moved = {{int16_t(block.first[0] + 1), int16_t(block.first[1] - 2), block.first[2]}};
    ASSERT_TRUE(got.count(moved) == 1);
    ASSERT_TRUE(std::memcmp(block.second, got.at(moved), sizeof(vk_voxel) * VK_BLOCK_VOXELS) == 0);
  }
}

// a wall fused in a frame of its own, merged into a fresh volume through a generic pose, seen from the camera carried along:
// the raycast finds the wall where the depth image had it. The resampled distance field is trilinear in a field that is
// close to linear across the surface, so its zero crossing moves by a fraction of a voxel: half a voxel bounds the mean.
TEST(MergePose, AGenericPoseThenARaycast)
{
  const Frame frame = SlantedFrame(Transform());
  auto source = Fused(8192, 2048, frame, 2);
  auto volume = std::make_shared<Volume>(8192, 4096);
  volume->SetVoxelLength(0.008f);
  const float yaw = 0.5f * 0.17453293f, pitch = 0.5f * 0.08726646f;   // 10 and 5 degrees
  const Transform pose = Transform::Translate(0.013f, -0.021f, 0.008f) * Transform::Rotate(std::cos(yaw), 0.0f, std::sin(yaw), 0.0f) *
      Transform::Rotate(std::cos(pitch), std::sin(pitch), 0.0f, 0.0f);
  const MergePoseCounts counts = volume->Merge(*source, pose);
  ASSERT_EQ(source->GetAllocatedBlockCount(), counts.considered);
  ASSERT_TRUE(counts.candidates > counts.considered);
  ASSERT_EQ(counts.candidates, counts.fused);
  ASSERT_EQ(counts.candidates, counts.allocated);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.sampled > 100000);
  ASSERT_EQ(counts.candidates, volume->GetAllocatedBlockCount());

  const Frame moved = SlantedFrame(pose);          // the same camera, in the destination's frame
  volume->SetView(moved, 3);
  Frame traced;
  traced.depth_to_world_transform = pose;
  traced.depth_projection = traced.color_projection = frame.depth_projection;
  traced.depth_image = std::make_shared<Image>(kWidth, kHeight);
  Tracer tracer(volume);
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
      error += std::fabs(depth - (1.5f + 0.001f * x + 0.0007f * y));
    }
  std::printf("         %d of %d pixels hit, mean |depth error| %.5f m\n", hits, kWidth * kHeight, hits ? error / hits : 0.0);
  ASSERT_TRUE(hits > kWidth * kHeight / 2);
  ASSERT_TRUE(error / hits < 0.004);
}

int main(int argc, char** argv) { return RunTests("merge_pose_tests", argc, argv); }
