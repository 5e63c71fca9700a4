// merge_tests.cpp — Volume::Merge through the C++ class layer -> C ABI -> HIP kernels (no upstream case: the reference's
// Volume is a process-wide singleton, src/volume.cu:17-21). The call's exact outcome is held against its CPU statement
// by tests/test_gpu_merge.py; these cases are what a user of the class sees: two volumes fused from different views
// become one map, a merge into a fresh volume copies the source, and the call refuses to run on top of an announced
// frame. Harness: volume_test_support.h.
//
//   ./merge_tests            run everything (needs a GPU)
//   ./merge_tests <filter>   run the cases whose name contains <filter>
#include "volume_test_support.h"

// two views of the same wall, each in a volume of its own: after the merge one volume holds both
TEST(Merge, TwoViewsBecomeOneMap)
{
  const Frame left = SlantedFrame(Transform());
  const Frame right = SlantedFrame(Transform::Translate(0.3f, 0.0f, 0.0f));
  auto a = Fused(8192, 2048, left, 2);
  auto b = Fused(4093, 4096, right, 3);            // another table size
  const int in_a = a->GetAllocatedBlockCount(), in_b = b->GetAllocatedBlockCount();
  ASSERT_TRUE(in_a > 500 && in_b > 500);
  const std::vector<vk_hash_entry> entries_a = Entries(*a), entries_b = Entries(*b);
  const std::vector<vk_voxel> voxels_a = Voxels(*a), voxels_b = Voxels(*b);
  const BlockMap before = Blocks(entries_a, voxels_a), source = Blocks(entries_b, voxels_b);
  int common = 0;
  for (const auto& block : source) common += before.count(block.first) ? 1 : 0;
  ASSERT_TRUE(common > 100 && common < in_b);

  const MergeCounts counts = a->Merge(*b);
  ASSERT_EQ(in_b, counts.considered);
  ASSERT_EQ(in_b, counts.fused);
  ASSERT_EQ(in_b - common, counts.allocated);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_EQ(0, counts.skipped);
  ASSERT_TRUE(counts.rounds >= 1);
  ASSERT_EQ(in_a + in_b - common, a->GetAllocatedBlockCount());
  ASSERT_EQ(in_b, b->GetAllocatedBlockCount());                     // the source is only read
  ASSERT_EQ(size_t(0), a->GetVisibleBlocks().GetSize());            // until the next SetView

  const std::vector<vk_hash_entry> entries_after = Entries(*a);
  const std::vector<vk_voxel> voxels_after = Voxels(*a);
  const BlockMap after = Blocks(entries_after, voxels_after);
  ASSERT_EQ(size_t(in_a + in_b - common), after.size());
  int summed = 0;
  for (const auto& block : after)
  {
    const bool was = before.count(block.first) != 0, comes = source.count(block.first) != 0;
    ASSERT_TRUE(was || comes);
    for (int i = 0; i < VK_BLOCK_VOXELS; ++i)
    {
      const int wa = was ? before.at(block.first)[i].distance_weight : 0;
      const int wb = comes ? source.at(block.first)[i].distance_weight : 0;
      ASSERT_EQ(wa + wb, block.second[i].distance_weight);          // 2 + 3 stays below the cap of 16
      if (wa && wb)
      {
        ++summed;
        const float da = before.at(block.first)[i].distance, db = source.at(block.first)[i].distance;
        const float want = (float(wa) * da + float(wb) * db) / (float(wa) + float(wb));
        ASSERT_TRUE(block.second[i].distance == want);
      }
    }
  }
  ASSERT_TRUE(summed > 1000);
  // the merged volume goes on: a view in between sees one map
  const Frame between = SlantedFrame(Transform::Translate(0.15f, 0.0f, 0.0f));
  a->SetView(between, 3);
  ASSERT_TRUE(a->GetVisibleBlocks().GetSize() > 500);
  DepthIntegrator integrator(a);
  integrator.Integrate(between);
}

// a fresh volume with another bucket count takes the source's blocks as they are
TEST(Merge, IntoAFreshVolumeIsACopy)
{
  const Frame frame = SlantedFrame(Transform());
  auto source = Fused(509, 4096, frame, 2);        // long chains: several rounds
  auto fresh = std::make_shared<Volume>(1021, 2048);
  fresh->SetVoxelLength(0.008f);
  const int blocks = source->GetAllocatedBlockCount();
  MergeOptions options;
  options.max_rounds = 2;                          // the class layer goes on until every block has had its rounds
  const MergeCounts counts = fresh->Merge(*source, options);
  ASSERT_EQ(blocks, counts.considered);
  ASSERT_EQ(blocks, counts.fused);
  ASSERT_EQ(blocks, counts.allocated);
  ASSERT_EQ(0, counts.left_out);
  ASSERT_TRUE(counts.rounds > 2);
  ASSERT_EQ(blocks, fresh->GetAllocatedBlockCount());
  const std::vector<vk_hash_entry> entries_s = Entries(*source), entries_f = Entries(*fresh);
  const std::vector<vk_voxel> voxels_s = Voxels(*source), voxels_f = Voxels(*fresh);
  const BlockMap want = Blocks(entries_s, voxels_s), got = Blocks(entries_f, voxels_f);
  ASSERT_EQ(want.size(), got.size());
  for (const auto& block : want)
  {
    ASSERT_TRUE(got.count(block.first) == 1);
    ASSERT_TRUE(std::memcmp(block.second, got.at(block.first), sizeof(vk_voxel) * VK_BLOCK_VOXELS) == 0);
  }
}

// between SetView calls only: not while Tracer::Trace(keyframe, next_frame) has the next frame's requests in either volume
TEST(Merge, RefusedWhileAFrameIsAnnounced)
{
  const Frame frame = SlantedFrame(Transform());
  auto volume = Fused(8192, 2048, frame, 1);
  auto other = Fused(8192, 2048, SlantedFrame(Transform::Translate(0.3f, 0.0f, 0.0f)), 1);
  Tracer tracer(volume);
  Frame keyframe;
  keyframe.depth_projection = frame.depth_projection;
  keyframe.depth_image = MakeDepth([](int, int) { return 0.0f; });
  Frame next = SlantedFrame(Transform::Translate(0.004f, 0.0f, 0.0f));
  tracer.Trace(keyframe, next);
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  const int before = volume->GetAllocatedBlockCount(), before_other = other->GetAllocatedBlockCount();
  ASSERT_THROW(volume->Merge(*other));             // as the destination
  ASSERT_THROW(other->Merge(*volume));             // and as the source
  ASSERT_THROW(other->Merge(*other));
  ASSERT_EQ(1, volume->GetRequestsAhead()->valid);
  ASSERT_EQ(before, volume->GetAllocatedBlockCount());
  ASSERT_EQ(before_other, other->GetAllocatedBlockCount());
  volume->CancelRequestsAhead(3);
  const int announced = volume->GetAllocatedBlockCount();
  const MergeCounts counts = volume->Merge(*other);
  ASSERT_EQ(before_other, counts.fused);
  ASSERT_EQ(announced + counts.allocated, volume->GetAllocatedBlockCount());
}

int main(int argc, char** argv) { return RunTests("merge_tests", argc, argv); }
